// The bodies of nxs_mapx_forward_point (nextsim_amd/csrc/nxs_mapx_body.inl) and of the nodal forcing kernels (nextsim_amd/csrc/nxs_nodal_forcing_kernels.inl)
// compiled for the HOST: the kernels' own source with the HIP qualifiers defined away, one call per thread of the launch grid, in the order nxs_dyn_forcing_ingest
// launches them.  tests/test_nodal_forcing_host_kernel.py builds it (g++ -O2 -ffp-contract=off) and requires the bits of the real forward_mapx and of the
// restated transformData as tests/golden/mapx_forward.npz holds them, and of the numpy expressions of the wrap and the blend.
//   usage: nodal_forcing_host_kernel IN OUT
//   IN (forward)  : int32[2] 0, n; double[15] nxs_mapx_polar; double[n] lat; double[n] lon                         OUT: double[n] x; double[n] y
//   IN (transform): int32[12] 1, M, N, N_data, npairs, per_point, rotate, cyclic_x, cyclic_y, 0, 0, 0; int32[4] j0; int32[4] j1; int32[4] east_west;
//                   double[15] nxs_mapx_polar; double[2] cos, sin(-rotation_angle); double[M] grid_y; double[M or M*N] lat; double[N or M*N] lon;
//                   double[M*N*N_data] data                                                                          OUT: double[cM*cN*N_data], -777 where nothing was written
//   IN (blend)    : int32[2] 2, Nn; 3 x { int32[2] mode, 0; double[4] fcoeff0, fcoeff1, factor, bias }; double[5*Nn] snapshot 0 (wind [2Nn], ocean [2Nn], ssh [Nn]);
//                   double[5*Nn] snapshot 1; double[5*Nn] the vectors before the launch                              OUT: double[5*Nn] the vectors after it
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
static constexpr int BLOCK = 256;
static struct { int x, y; } blockIdx, threadIdx;
#include "nxs_dyn.h"
#include "nxs_interp.h"
#include "nxs_grid_to_mesh_body.inl"
#include "nxs_nodal_forcing_kernels.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return fread(p, size, n, f) == n; }
static int nblocks(int n) { return n > 0 ? (n + BLOCK - 1) / BLOCK : 1; }
static int put(const char *path, const std::vector<double> &v) {
    FILE *g = fopen(path, "wb");
    if (!g) return 5;
    fwrite(v.data(), 8, v.size(), g);
    fclose(g);
    return 0;
}
template <class F> static void launch(int gx, int gy, F f) {
    for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < gx; ++bx)
            for (int tx = 0; tx < BLOCK; ++tx) { blockIdx.x = bx; blockIdx.y = by; threadIdx.x = tx; f(); }
}

static int forward(FILE *f, int n, const char *out_path) {
    nxs_mapx_polar m;
    std::vector<double> lat(n), lon(n), xy(2 * (size_t)n);
    if (!rd(f, &m, 8, 15) || !rd(f, lat.data(), 8, n) || !rd(f, lon.data(), 8, n)) return 4;
    launch(nblocks(n), 1, [&] { k_mapx_forward(m, n, lat.data(), lon.data(), xy.data(), xy.data() + n); });
    return put(out_path, xy);
}

static int transform(FILE *f, const int *hdr, const char *out_path) {
    const int M = hdr[1], N = hdr[2], ND = hdr[3], npairs = hdr[4], per_point = hdr[5], rotate = hdr[6], cx = hdr[7], cy = hdr[8];
    if (npairs < 0 || npairs > NF_MAX_VECTORS || ND < 1 || ND > NF_MAX_COLUMNS || M < 2 || N < 2) return 6;
    const int cM = M + (cy ? 1 : 0), cN = N + (cx ? 1 : 0);
    NfVectors a{};
    double cs[2];
    std::vector<double> gy(M), lat(per_point ? (size_t)M * N : M), lon(per_point ? (size_t)M * N : N), in((size_t)M * N * ND), data((size_t)cM * cN * ND, -777.);
    if (!rd(f, a.j0, 4, 4) || !rd(f, a.j1, 4, 4) || !rd(f, a.east_west, 4, 4) || !rd(f, &a.map, 8, 15) || !rd(f, cs, 8, 2) || !rd(f, gy.data(), 8, M) ||
        !rd(f, lat.data(), 8, lat.size()) || !rd(f, lon.data(), 8, lon.size()) || !rd(f, in.data(), 8, in.size()))
        return 4;
    for (int y = 0; y < M; ++y)   // the upload: rows of N cells into rows of cN
        for (size_t q = 0; q < (size_t)N * ND; ++q) data[((size_t)y * cN) * ND + q] = in[((size_t)y * N) * ND + q];
    a.g = NfGrid{data.data(), M, N, cM, cN, ND};
    a.npairs = npairs;
    a.lat = lat.data(); a.lon = lon.data(); a.per_point = per_point;
    a.pole_row = a.pole_next = -1;
    if (gy[0] == 90.) { a.pole_row = 0; a.pole_next = 1; }
    if (gy[M - 1] == 90.) { a.pole_row = M - 1; a.pole_next = M - 2; }
    a.R = NXS_MAPX_RE_KM * 1000.;
    a.c = cs[0]; a.s = cs[1];
    bool any = false;
    for (int k = 0; k < npairs; ++k) any = any || a.east_west[k];
    if (npairs > 0 && any) {
        launch(nblocks(M * N), npairs, [&] { k_nf_east_north(a); });
        if (a.pole_row >= 0) launch(1, 1, [&] { k_nf_pole(a); });
    }
    if (npairs > 0 && rotate) launch(nblocks(M * N), npairs, [&] { k_nf_rotate(a); });
    if (cx || cy) launch(nblocks((cx ? M : 0) + (cy ? N : 0) + 1), 1, [&] { k_nf_wrap(a.g); });
    return put(out_path, data);
}

static int blend(FILE *f, int Nn, const char *out_path) {
    int mode[NF_GROUPS];
    double par[NF_GROUPS][4];
    for (int k = 0; k < NF_GROUPS; ++k) {
        int m[2];
        if (!rd(f, m, 4, 2) || !rd(f, par[k], 8, 4)) return 4;
        mode[k] = m[0];
    }
    const size_t n = 5 * (size_t)Nn, off[NF_GROUPS] = {0, 2 * (size_t)Nn, 4 * (size_t)Nn};
    // every vector an allocation of its own, as on the device: each starts 16-byte aligned
    std::vector<double> d0[NF_GROUPS], d1[NF_GROUPS], out[NF_GROUPS], all(n);
    for (auto *set : {d0, d1, out}) {
        if (!rd(f, all.data(), 8, n)) return 4;
        for (int k = 0; k < NF_GROUPS; ++k) set[k].assign(all.begin() + off[k], all.begin() + off[k] + (k < 2 ? 2 : 1) * (size_t)Nn);
    }
    NfBlend b{};
    b.Nn = Nn;
    for (int k = 0; k < NF_GROUPS; ++k) {
        if (mode[k] == NXS_TF_OFF) continue;
        b.grp[b.ngroups++] = NfGroup{d0[k].data(), mode[k] == NXS_TF_LINEAR ? d1[k].data() : nullptr, out[k].data(), k < 2 ? 2 : 1, par[k][0], par[k][1], par[k][2], par[k][3], mode[k]};
    }
    if (b.ngroups) launch(nblocks((Nn + 1) / 2), b.ngroups, [&] { k_nf_blend(b); });
    for (int k = 0; k < NF_GROUPS; ++k) std::copy(out[k].begin(), out[k].end(), all.begin() + off[k]);
    return put(out_path, all);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[12] = {0};
    if (!rd(f, hdr, 4, 2)) return 4;
    int rc;
    if (hdr[0] == 0) rc = forward(f, hdr[1], argv[2]);
    else if (hdr[0] == 2) rc = blend(f, hdr[1], argv[2]);
    else rc = rd(f, hdr + 2, 4, 10) ? transform(f, hdr, argv[2]) : 4;
    fclose(f);
    return rc;
}
