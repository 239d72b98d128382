// The device code of the coupler's put compiled for the HOST: the body of the send kernel (nxs_remap::grid_values<NV>, nextsim_amd/csrc/nxs_remap_core.inl) inside
// the loop k_gridmap_send and nxs_gridmap_send_rows make around it (one pass per cell, column tiles of 12, the builds for at most 4, 8 and 12 variables), and
// D_dmax / D_dmean (nextsim_amd/csrc/nxs_fsd_diag_body.inl).  tests/test_cpl_out_host_kernel.py builds it (g++ -O2 -ffp-contract=off) and requires the bits of
// tests/cpl_out_ref.py; the same program is run once under -fsanitize=address,undefined.
//   usage: cpl_out_host_kernel MODE IN OUT
//   send  IN : int32[5] nels, G, rows, n, n_el; int32[rows] gridP; int32[rows + 1] off; int32[n] tris; double[n] w; double[4 G] cornerX, cornerY;
//              double[nels][n_el] the mesh accumulators; double[n_el][G] data_grid          OUT: double[n_el][G] data_grid
//   fsd   IN : int32[2] nb, n; double[3] dmax_c_threshold, fsd_unbroken_floe_size, fsd_min_floe_size; double[16] up; double[16] centres; double[nb][n] mech;
//              double[n] D_conc                                                              OUT: double[n] D_dmax, double[n] D_dmean
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define NXS_HD
#define __host__
#define __device__
#include "nxs_remap_core.inl"
#include "nxs_fsd_diag_body.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }

template <int NV>
static void send_tile(int G, int nb_var, int col0, int nv, const int *row_of_cell, const int *off, const int *tris, const double *w, const double *r_area, const double *in,
                      double *data_grid) {
    for (int c = 0; c < G; ++c) {   // k_gridmap_send, one thread
        const int row = row_of_cell[c];
        double v[NV];
        if (row < 0) {
            for (int i = 0; i < NV; ++i) v[i] = 0.;
        } else {
            const int lo = off[row];
            nxs_remap::grid_values<NV>(in, nb_var, col0, nv, tris + lo, w + lo, off[row + 1] - lo, r_area[row], v);
        }
        for (int i = 0; i < NV; ++i)
            if (i < nv) data_grid[(size_t)(col0 + i) * G + c] += v[i];
    }
}

static int send(FILE *f, FILE *g) {
    int hdr[5];
    if (!rd(f, hdr, 4, 5)) return 4;
    const int nels = hdr[0], G = hdr[1], rows = hdr[2], n = hdr[3], n_el = hdr[4];
    if (nels < 1 || G < 1 || rows < 0 || n < 0 || n_el < 1) return 6;
    std::vector<int> gridP(rows), off((size_t)rows + 1), tris(n), row_of_cell(G, -1);
    std::vector<double> w(n), cx(4 * (size_t)G), cy(4 * (size_t)G), in((size_t)nels * n_el), grid((size_t)n_el * G), r_area(rows);
    if (!rd(f, gridP.data(), 4, rows) || !rd(f, off.data(), 4, off.size()) || !rd(f, tris.data(), 4, n) || !rd(f, w.data(), 8, n) || !rd(f, cx.data(), 8, cx.size()) ||
        !rd(f, cy.data(), 8, cy.size()) || !rd(f, in.data(), 8, in.size()) || !rd(f, grid.data(), 8, grid.size()))
        return 4;
    for (int i = 0; i < rows; ++i) {   // k_gridmap_rows
        r_area[i] = nxs_remap::r_cell_area_n<4>(cx.data() + 4 * (size_t)gridP[i], cy.data() + 4 * (size_t)gridP[i]);
        row_of_cell[gridP[i]] = i;
    }
    for (int col0 = 0; col0 < n_el; col0 += 12) {   // nxs_gridmap_send_rows
        const int nv = std::min(12, n_el - col0);
        if (nv <= 4) send_tile<4>(G, n_el, col0, nv, row_of_cell.data(), off.data(), tris.data(), w.data(), r_area.data(), in.data(), grid.data());
        else if (nv <= 8) send_tile<8>(G, n_el, col0, nv, row_of_cell.data(), off.data(), tris.data(), w.data(), r_area.data(), in.data(), grid.data());
        else send_tile<12>(G, n_el, col0, nv, row_of_cell.data(), off.data(), tris.data(), w.data(), r_area.data(), in.data(), grid.data());
    }
    fwrite(grid.data(), 8, grid.size(), g);
    return 0;
}

static int fsd(FILE *f, FILE *g) {
    int hdr[2];
    double opt[3];
    nxs_fsd_diag::Args a{};
    if (!rd(f, hdr, 4, 2) || !rd(f, opt, 8, 3) || !rd(f, a.up, 8, 16) || !rd(f, a.centres, 8, 16)) return 4;
    const int nb = hdr[0], n = hdr[1];
    if (nb < 0 || nb > nxs_fsd_diag::MAX_BINS || n < 1) return 6;
    std::vector<double> mech((size_t)nb * n), conc(n), dmax(n), dmean(n);
    if (!rd(f, mech.data(), 8, mech.size()) || !rd(f, conc.data(), 8, n)) return 4;
    a.mech = mech.data(); a.stride = n; a.nb = nb;
    a.dmax_c_threshold = opt[0]; a.unbroken_floe_size = opt[1]; a.min_floe_size = opt[2];
    for (int i = 0; i < n; ++i) nxs_fsd_diag::diag(a, i, conc[i], dmax[i], dmean[i]);
    fwrite(dmax.data(), 8, n, g);
    fwrite(dmean.data(), 8, n, g);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 3;
    FILE *g = fopen(argv[3], "wb");
    if (!g) { fclose(f); return 5; }
    int rc = 2;
    if (!strcmp(argv[1], "send")) rc = send(f, g);
    else if (!strcmp(argv[1], "fsd")) rc = fsd(f, g);
    fclose(f);
    fclose(g);
    return rc;
}
