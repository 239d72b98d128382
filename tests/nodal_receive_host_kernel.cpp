// The bodies of the three node-map kernels (nextsim_amd/csrc/nxs_nodemap_kernels.inl: k_nodemap_weights, k_nodemap_source, k_nodemap_gather) compiled for the HOST:
// the kernels' own source with the HIP qualifiers defined away, one call per thread of the launch grid.  The weights kernel runs on tables made by the library's
// own host code (nxs_hull.inl: bamg's integer plane and convex completion) and a brute-force locator of the test's own (below), which tries every triangle in
// ascending number -- the order the device's locate() tests its candidates in.  tests/test_nodal_receive_host_kernel.py builds it twice (g++ -O2 -ffp-contract=off; the same with
// -fsanitize=address,undefined), every array an allocation of exactly its size, and compares with tests/golden/nodal_receive.npz.
//   usage: nodal_receive_host_kernel IN OUT
//   IN (weights): int32[4] 0, nods, nels, N; int32[3*nels] tri (0-based); double[nods] x, y; double[N] px, py
//                 OUT: double[3*N] v0, v1, v2; double[3*N] a0, a1, a2; double[4] counts (in a fill triangle, the first of them, beyond the hull, lost)
//   IN (receive): int32[16] 1, G, R, N, n_var, npairs, j0[2], j1[2], east_west, rotate, get, has_reduced, 0, 0; double[4] a, b, factor, bias; double[2] c, s;
//                 double[15] nxs_mapx_polar; int32[R] reduced; double[R] cs, sn, lat, lon; double[n_var*G] fields; int32[N] v0, v1, v2; double[N] a0, a1, a2
//                 OUT: double[n_var*R] loaded_data; double[n_var*N] the rows
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
static struct { int x, y; } blockIdx, threadIdx;
static int atomicAdd(int *p, int v) { const int o = *p; *p += v; return o; }
static int atomicMin(int *p, int v) { const int o = *p; if (v < o) *p = v; return o; }
#include "nxs_dyn.h"
#include "nxs_interp.h"
#include "nxs_hull.inl"

// The device's locator (locate() of nxs_interp.hip, bucket grid and all) is not part of this program: the test supplies the SAME CONTRACT by brute force -- bamg's
// R2ToI2 (truncation of coefIcoor*(P - pmin), Mesh.cpp:3688-3690), then every triangle of the completed mesh in ascending number, the first whose three integer
// area coordinates (det.h:8-12) are >= 0 with a positive sum -- as tests/drifters_ref.locate states it in numpy.  What is compiled from the library is the
// weights kernel itself: the division, the hull projection and the slot placement.
struct HullDev { int a, b, tri, k; };
struct InterpDev {
    int nods, nels, nels_all, N_interp, nodal, nhull;
    const HullDev *hull;
    const int *t0, *t1, *t2, *ix, *iy;
    double coef, pminx, pminy;
};
static inline long long det3(long long ax, long long ay, long long bx, long long by, long long cx, long long cy) { return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax); }
static inline int locate(const InterpDev &d, double x, double y, long long dd[3], long long &Bx, long long &By) {
    Bx = (long long)(int)(d.coef * (x - d.pminx));
    By = (long long)(int)(d.coef * (y - d.pminy));
    for (int t = 0; t < d.nels_all; ++t) {
        const int v0 = d.t0[t], v1 = d.t1[t], v2 = d.t2[t];
        const long long e0 = det3(d.ix[v1], d.iy[v1], d.ix[v2], d.iy[v2], Bx, By), e1 = det3(d.ix[v2], d.iy[v2], d.ix[v0], d.iy[v0], Bx, By),
                        e2 = det3(d.ix[v0], d.iy[v0], d.ix[v1], d.iy[v1], Bx, By);
        if (e0 >= 0 && e1 >= 0 && e2 >= 0 && e0 + e1 + e2 > 0) { dd[0] = e0; dd[1] = e1; dd[2] = e2; return t; }
    }
    return -1;
}
#include "nxs_nodemap_kernels.inl"

static bool rd(FILE *f, void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }
static int nblocks(int n) { return n > 0 ? (n + 255) / 256 : 1; }
static int put(const char *path, const std::vector<double> &v) {
    FILE *g = fopen(path, "wb");
    if (!g) return 5;
    fwrite(v.data(), 8, v.size(), g);
    fclose(g);
    return 0;
}
template <class F> static void launch(int gx, F f) {
    for (int bx = 0; bx < gx; ++bx)
        for (int tx = 0; tx < 256; ++tx) { blockIdx.x = bx; threadIdx.x = tx; f(); }
}

static int weights(FILE *f, const int *hdr, const char *out_path) {
    const int nods = hdr[1], nels = hdr[2], N = hdr[3];
    if (nods < 3 || nels < 1 || N < 1) return 6;
    std::vector<int> tri(3 * (size_t)nels);
    std::vector<double> x(nods), y(nods), px(N), py(N);
    if (!rd(f, tri.data(), 4, tri.size()) || !rd(f, x.data(), 8, nods) || !rd(f, y.data(), 8, nods) || !rd(f, px.data(), 8, N) || !rd(f, py.data(), 8, N)) return 4;
    std::vector<int> ix, iy, index1(tri);
    for (int &v : index1) v += 1;
    InterpDev d{};
    if (!nxs_hull::int_plane(x.data(), y.data(), nods, ix, iy, d.coef, d.pminx, d.pminy)) return 7;
    const nxs_hull::Completion comp = nxs_hull::complete_any(index1.data(), ix.data(), iy.data(), nods, nels);
    if (!comp.ok) return 8;
    const int nfill = (int)comp.fill.size() / 3, nall = nels + nfill;
    std::vector<int> t0(nall), t1(nall), t2(nall);
    for (int e = 0; e < nall; ++e) {
        const int *t = e < nels ? &tri[3 * (size_t)e] : &comp.fill[3 * (size_t)(e - nels)];
        t0[e] = t[0]; t1[e] = t[1]; t2[e] = t[2];
    }
    std::vector<HullDev> hull;
    for (const auto &h : comp.hull) hull.push_back(HullDev{h.a, h.b, h.tri, h.k});
    d.nods = nods; d.nels = nels; d.nels_all = nall; d.N_interp = N; d.nodal = 1;
    d.nhull = (int)hull.size(); d.hull = hull.data();
    d.t0 = t0.data(); d.t1 = t1.data(); d.t2 = t2.data(); d.ix = ix.data(); d.iy = iy.data();
    std::vector<int> v0(N), v1(N), v2(N), counts{0, INT_MAX, 0, 0};
    std::vector<double> a0(N), a1(N), a2(N);
    launch(nblocks(N), [&] { nodemap::k_nodemap_weights(d, px.data(), py.data(), nodemap::Weights{v0.data(), v1.data(), v2.data(), a0.data(), a1.data(), a2.data()}, counts.data()); });
    std::vector<double> out;
    for (const auto *v : {&v0, &v1, &v2}) out.insert(out.end(), v->begin(), v->end());
    for (const auto *a : {&a0, &a1, &a2}) out.insert(out.end(), a->begin(), a->end());
    out.insert(out.end(), counts.begin(), counts.end());
    return put(out_path, out);
}

static int receive(FILE *f, const int *hdr, const char *out_path) {
    const int G = hdr[1], R = hdr[2], N = hdr[3], n_var = hdr[4], npairs = hdr[5], east_west = hdr[10], rotate = hdr[11], get = hdr[12], has_reduced = hdr[13];
    if (G < 1 || R < 1 || R > G || N < 1 || n_var < 1 || n_var > nodemap::kMaxVar || npairs < 0 || npairs > nodemap::kMaxPairs) return 6;
    nodemap::SourceArgs s{};
    nodemap::GatherArgs g{};
    double cs2[2];
    if (!rd(f, s.a, 8, 4) || !rd(f, s.b, 8, 4) || !rd(f, g.factor, 8, 4) || !rd(f, g.bias, 8, 4) || !rd(f, cs2, 8, 2) || !rd(f, &s.map, 8, 15)) return 4;
    std::vector<int> reduced(R), v0(N), v1(N), v2(N);
    std::vector<double> cs(R), sn(R), lat(R), lon(R), fields((size_t)n_var * G), a0(N), a1(N), a2(N);
    if (!rd(f, reduced.data(), 4, R) || !rd(f, cs.data(), 8, R) || !rd(f, sn.data(), 8, R) || !rd(f, lat.data(), 8, R) || !rd(f, lon.data(), 8, R) ||
        !rd(f, fields.data(), 8, fields.size()) || !rd(f, v0.data(), 4, N) || !rd(f, v1.data(), 4, N) || !rd(f, v2.data(), 4, N) || !rd(f, a0.data(), 8, N) ||
        !rd(f, a1.data(), 8, N) || !rd(f, a2.data(), 8, N))
        return 4;
    std::vector<std::vector<double>> field(n_var), row(n_var);      // every field and row an allocation of its own, as a coupler delivers them
    std::vector<double> stage((size_t)n_var * R, -777.);
    for (int v = 0; v < n_var; ++v) {
        field[v].assign(fields.begin() + (size_t)v * G, fields.begin() + (size_t)(v + 1) * G);
        row[v].assign(N, -777.);
        s.field[v] = field[v].data();
        g.out[v] = row[v].data();
    }
    s.n_var = n_var; s.R = R; s.reduced = has_reduced ? reduced.data() : nullptr;
    s.npairs = npairs;
    for (int k = 0; k < 2; ++k) { s.j0[k] = hdr[6 + k]; s.j1[k] = hdr[8 + k]; }
    s.east_west = east_west; s.lat = lat.data(); s.lon = lon.data(); s.Re = NXS_MAPX_RE_KM * 1000.;
    s.rotate = rotate; s.c = cs2[0]; s.s = cs2[1]; s.cs = cs.data(); s.sn = sn.data();
    s.stage = stage.data();
    g.stage = stage.data(); g.R = R; g.N = N; g.get = get;
    launch(nblocks(R), [&] { nodemap::k_nodemap_source(s); });
    auto gather = [&](auto nv) {
        launch(nblocks(N), [&] { nodemap::k_nodemap_gather<decltype(nv)::value>(g, v0.data(), v1.data(), v2.data(), a0.data(), a1.data(), a2.data()); });
    };
    switch (n_var) {
        case 1: gather(std::integral_constant<int, 1>{}); break;
        case 2: gather(std::integral_constant<int, 2>{}); break;
        case 3: gather(std::integral_constant<int, 3>{}); break;
        default: gather(std::integral_constant<int, 4>{}); break;
    }
    std::vector<double> out(stage);
    for (int v = 0; v < n_var; ++v) out.insert(out.end(), row[v].begin(), row[v].end());
    return put(out_path, out);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int hdr[16] = {0};
    if (!rd(f, hdr, 4, 4)) return 4;
    int rc;
    if (hdr[0] == 0) rc = weights(f, hdr, argv[2]);
    else rc = rd(f, hdr + 4, 4, 12) ? receive(f, hdr, argv[2]) : 4;
    fclose(f);
    return rc;
}
