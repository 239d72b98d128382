// The bodies of the two load kernels (nextsim_amd/csrc/nxs_nodemap_load_kernels.inl: k_nodemap_load, k_nodemap_cols_gather) compiled for the HOST: the kernels' own
// source with the HIP qualifiers defined away, one call per thread of the launch grid.  tests/test_mesh_forcing_host_kernel.py builds it twice (g++ -O2
// -ffp-contract=off; the same with -fsanitize=address,undefined), every array an allocation of exactly its size, and compares with tests/golden/mesh_forcing.npz.
//   usage: mesh_forcing_host_kernel IN OUT
//   IN:  int32[16] G, R, N, n_var, n_step, npairs, j0[2], j1[2], east_west, rotate, has_reduced, keep (bit c: column c is gathered), 0, 0;
//        double[8] scale_factor, add_offset, a, b; double[2] c, s; double[15] nxs_mapx_polar; int32[R] reduced; double[R] cs, sn, lat, lon;
//        double[n_cols*G] fields; int32[N] v0, v1, v2; double[N] a0, a1, a2
//   OUT: double[n_cols*R] loaded_data; double[kept*N] the kept rows in column order
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <type_traits>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
static struct { int x, y; } blockIdx, threadIdx;
#include "nxs_dyn.h"
#include "nxs_interp.h"
#include "nxs_east_north_body.inl"
namespace nodemap {
enum { kMaxVar = 4, kMaxPairs = 2 };                                         // nxs_nodemap_kernels.inl's, which the load kernels' file continues
enum { ROTATE_NONE = 0, ROTATE_UNIFORM = 1, ROTATE_GRID_THETA = 2 };
}  // namespace nodemap
#include "nxs_nodemap_load_kernels.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }
static int nblocks(int n) { return n > 0 ? (n + 255) / 256 : 1; }
template <class F> static void launch(int gx, F f) {
    for (int bx = 0; bx < gx; ++bx)
        for (int tx = 0; tx < 256; ++tx) { blockIdx.x = bx; threadIdx.x = tx; f(); }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[16] = {0};
    if (!rd(f, hdr, 4, 16)) return 4;
    const int G = hdr[0], R = hdr[1], N = hdr[2], n_var = hdr[3], n_step = hdr[4], npairs = hdr[5], east_west = hdr[10], rotate = hdr[11], has_reduced = hdr[12], keep = hdr[13];
    const int n_cols = n_var * n_step;
    if (G < 1 || R < 1 || R > G || N < 1 || n_var < 1 || n_var > nodemap::kMaxVar || n_step < 1 || n_step > 2 || npairs < 0 || npairs > nodemap::kMaxPairs) return 6;
    nodemap::LoadArgs s{};
    nodemap::ColsArgs g{};
    double cs2[2];
    if (!rd(f, s.scale_factor, 8, 8) || !rd(f, s.add_offset, 8, 8) || !rd(f, s.a, 8, 8) || !rd(f, s.b, 8, 8) || !rd(f, cs2, 8, 2) || !rd(f, &s.map, 8, 15)) return 4;
    std::vector<int> reduced(R), v0(N), v1(N), v2(N);
    std::vector<double> cs(R), sn(R), lat(R), lon(R), fields((size_t)n_cols * G), a0(N), a1(N), a2(N);
    if (!rd(f, reduced.data(), 4, R) || !rd(f, cs.data(), 8, R) || !rd(f, sn.data(), 8, R) || !rd(f, lat.data(), 8, R) || !rd(f, lon.data(), 8, R) ||
        !rd(f, fields.data(), 8, fields.size()) || !rd(f, v0.data(), 4, N) || !rd(f, v1.data(), 4, N) || !rd(f, v2.data(), 4, N) || !rd(f, a0.data(), 8, N) ||
        !rd(f, a1.data(), 8, N) || !rd(f, a2.data(), 8, N))
        return 4;
    fclose(f);
    std::vector<std::vector<double>> field(n_cols), row;      // every field and row an allocation of its own
    std::vector<double> stage((size_t)n_cols * R, -777.);
    int kept = 0;
    for (int c = 0; c < n_cols; ++c) {
        field[c].assign(fields.begin() + (size_t)c * G, fields.begin() + (size_t)(c + 1) * G);
        s.field[c] = field[c].data();
        if (keep & (1 << c)) { g.col[kept++] = c; row.emplace_back(N, -777.); }
    }
    if (kept < 1) return 6;
    for (int k = 0; k < kept; ++k) g.out[k] = row[k].data();
    s.n_var = n_var; s.n_step = n_step; s.R = R; s.reduced = has_reduced ? reduced.data() : nullptr;
    s.npairs = npairs;
    for (int k = 0; k < 2; ++k) { s.j0[k] = hdr[6 + k]; s.j1[k] = hdr[8 + k]; }
    s.east_west = east_west; s.lat = lat.data(); s.lon = lon.data(); s.Re = NXS_MAPX_RE_KM * 1000.;
    s.rotate = rotate; s.c = cs2[0]; s.s = cs2[1]; s.cs = cs.data(); s.sn = sn.data();
    s.stage = stage.data();
    g.stage = stage.data(); g.R = R; g.N = N;
    launch(nblocks(R), [&] { nodemap::k_nodemap_load(s); });
    auto gather = [&](auto nc) {
        launch(nblocks(N), [&] { nodemap::k_nodemap_cols_gather<decltype(nc)::value>(g, v0.data(), v1.data(), v2.data(), a0.data(), a1.data(), a2.data()); });
    };
    switch (kept) {
        case 1: gather(std::integral_constant<int, 1>{}); break;
        case 2: gather(std::integral_constant<int, 2>{}); break;
        case 3: gather(std::integral_constant<int, 3>{}); break;
        case 4: gather(std::integral_constant<int, 4>{}); break;
        case 5: gather(std::integral_constant<int, 5>{}); break;
        case 6: gather(std::integral_constant<int, 6>{}); break;
        case 7: gather(std::integral_constant<int, 7>{}); break;
        default: gather(std::integral_constant<int, 8>{}); break;
    }
    std::vector<double> out(stage);
    for (int k = 0; k < kept; ++k) out.insert(out.end(), row[k].begin(), row[k].end());
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 5;
    fwrite(out.data(), 8, out.size(), o);
    fclose(o);
    return 0;
}
