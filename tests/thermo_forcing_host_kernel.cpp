// The bodies of k_thermo_forcing_blend and k_thermo_forcing_ingest (nextsim_amd/csrc/nxs_thermo_forcing_kernels.inl, with nxs_grid_to_mesh_body.inl: the arithmetic
// nxs_interp_grid_to_mesh runs) compiled for the HOST: the kernels' own source with the HIP qualifiers defined away, one call per thread of the launch grid.
// tests/test_thermo_forcing_host_kernel.py builds it (g++ -O2 -ffp-contract=off) and requires the bits of the numpy expression (blend) and of the real bamg's golden
// file (ingest): the transcription is then checked without a device.
//   usage: thermo_forcing_host_kernel IN OUT
//   IN (blend) : int32[2] 0, Ne; 10 x { int32[2] mode, 0; double[4] fcoeff0, fcoeff1, factor, bias }; double[10][Ne] snapshot 0; double[10][Ne] snapshot 1;
//                double[10][Ne] the rows before the launch
//   OUT        : double[10][Ne] the rows after it (the table is packed as nxs_dyn_thermo_forcing_time packs it: an OFF row is not in it)
//   IN (ingest): int32[10] 1, Ne, M, N, N_data, x_rows, y_rows, interp, row_major, 0; double default_value; double[x_rows] x_in; double[y_rows] y_in;
//                double[M*N*N_data] data; double[Ne] RX; double[Ne] RY; int32[N_data] row; int32[N_data] snapshot
//   OUT        : double[2][10][Ne] the snapshots, -777 where nothing was written
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
#include "nxs_interp.h"
#include "nxs_thermo_forcing_kernels.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return fread(p, size, n, f) == n; }
static int nblocks(int n) { return n > 0 ? (n + BLOCK - 1) / BLOCK : 1; }

static int blend(FILE *f, int Ne, const char *out_path) {
    int mode[TF_ROWS];
    double par[TF_ROWS][4];
    for (int k = 0; k < TF_ROWS; ++k) {
        int m[2];
        if (!rd(f, m, 4, 2) || !rd(f, par[k], 8, 4)) return 4;
        mode[k] = m[0];
    }
    std::vector<double> d0((size_t)TF_ROWS * Ne), d1(d0.size()), out(d0.size());
    if (!rd(f, d0.data(), 8, d0.size()) || !rd(f, d1.data(), 8, d1.size()) || !rd(f, out.data(), 8, out.size())) return 4;
    TfBlend b{};
    b.Ne = Ne;
    for (int k = 0; k < TF_ROWS; ++k) {
        if (mode[k] == NXS_TF_OFF) continue;
        b.row[b.nrows++] = TfRow{d0.data() + (size_t)k * Ne, d1.data() + (size_t)k * Ne, out.data() + (size_t)k * Ne, par[k][0], par[k][1], par[k][2], par[k][3], mode[k]};
    }
    const int gx = nblocks((Ne + 1) / 2);
    for (int by = 0; by < b.nrows; ++by)
        for (int bx = 0; bx < gx; ++bx)
            for (int tx = 0; tx < BLOCK; ++tx) { blockIdx.x = bx; blockIdx.y = by; threadIdx.x = tx; k_thermo_forcing_blend(b); }
    FILE *g = fopen(out_path, "wb");
    if (!g) return 5;
    fwrite(out.data(), 8, out.size(), g);
    fclose(g);
    return 0;
}

static int ingest(FILE *f, const int *hdr, const char *out_path) {
    const int Ne = hdr[1], M = hdr[2], N = hdr[3], N_data = hdr[4], x_rows = hdr[5], y_rows = hdr[6], interp = hdr[7], row_major = hdr[8];
    if (N_data < 1 || N_data > TF_MAX_COLUMNS) return 6;
    double default_value;
    if (!rd(f, &default_value, 8, 1)) return 4;
    std::vector<double> x_in(x_rows), y_in(y_rows), data((size_t)M * N * N_data), rx(Ne), ry(Ne);
    std::vector<int32_t> row(N_data), snap(N_data);
    if (!rd(f, x_in.data(), 8, x_in.size()) || !rd(f, y_in.data(), 8, y_in.size()) || !rd(f, data.data(), 8, data.size()) || !rd(f, rx.data(), 8, Ne) || !rd(f, ry.data(), 8, Ne) ||
        !rd(f, row.data(), 4, N_data) || !rd(f, snap.data(), 4, N_data))
        return 4;
    std::vector<double> x(N), y(M);
    if (!g2m_centres(x_in.data(), x_rows, y_in.data(), y_rows, M, N, x.data(), y.data())) return 7;
    std::vector<double> out((size_t)2 * TF_ROWS * Ne, -777.);
    TfIngest a{};
    a.g = G2M{x.data(), y.data(), N, M, M, N, N_data, Ne, interp, row_major != 0, g2m_monotone(x.data(), N), g2m_monotone(y.data(), M), default_value};
    a.rx = rx.data(); a.ry = ry.data();
    for (int j = 0; j < N_data; ++j)
        if (row[j] >= 0) a.dst[j] = out.data() + ((size_t)snap[j] * TF_ROWS + row[j]) * Ne;
    for (int bx = 0; bx < nblocks(Ne); ++bx)
        for (int tx = 0; tx < BLOCK; ++tx) { blockIdx.x = bx; blockIdx.y = 0; threadIdx.x = tx; k_thermo_forcing_ingest(a, data.data()); }
    FILE *g = fopen(out_path, "wb");
    if (!g) return 5;
    fwrite(out.data(), 8, out.size(), g);
    fclose(g);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[10] = {0};
    if (!rd(f, hdr, 4, 2)) return 4;
    int rc;
    if (hdr[0] == 0) rc = blend(f, hdr[1], argv[2]);
    else rc = rd(f, hdr + 2, 4, 8) ? ingest(f, hdr, argv[2]) : 4;
    fclose(f);
    return rc;
}
