// nxs_nodemap_kernels.inl -- the coupler's receive of NODAL fields through weights computed once per mesh (include/nxs_interp.h, nxs_nodemap_*).  Textually included
// by nxs_interp.hip inside its unnamed namespace, behind locate().  bamg = contrib/bamg/src, externaldata.cpp = model/externaldata.cpp.
//   k_nodemap_weights   InterpFromMeshToMesh2dx_weights.cpp:59-120 for nodal data, one thread per target: locate() (the integers of k_interp), (double)dete[k]/tb.det
//              inside a triangle of the source; beyond the hull CloseBoundaryEdge's edge or vertex outcome placed by VerticesOfTriangularEdge / OppositeVertex in the
//              triangle behind the hull edge.  Six SoA rows out.  A target in a fill triangle (reft < 0, :72-73) is COUNTED, its rows left alone: the caller refuses.
//   k_nodemap_source    one thread per reduced source point: receiveCouplingData's  t = field[reduced[i]]; t *= a; t += b  (externaldata.cpp:498-509), then
//              transformData per pair on the point's own two entries: the east/north branch (nf_east_north_point, nxs_east_north_body.inl), then the uniform
//              (:1246-1261) or the per-point rotation (:1263-1281, cos / sin rows made on the host).  Rows [n_var][R] of the map's staging buffer.
//   k_nodemap_gather<NV>  InterpFromMeshToMesh2dx_apply.cpp:57-59, one thread per target: three vertices and three weights loaded once, per variable
//              a0*d[v0] + a1*d[v1] + a2*d[v2] left to right, then ExternalData::get's factor*x + bias (externaldata.cpp:434, 438) where asked.  Consecutive threads
//              read consecutive entries of the six rows and store consecutive entries of each output row.  No atomics, no LDS, no scratch.
// The bodies compile for the host (tests/nodal_receive_host_kernel.cpp defines the HIP qualifiers away, and supplies a brute-force locate() for the weights kernel).  The build is uncontracted (-ffp-contract=off).

#include "nxs_east_north_body.inl"

namespace nodemap {

enum { kMaxVar = 4, kMaxPairs = 2 };
enum { ROTATE_NONE = 0, ROTATE_UNIFORM = 1, ROTATE_GRID_THETA = 2 };
enum { OUT_INSIDE = 0, OUT_HULL = 1, OUT_FILL = -1, OUT_LOST = -2 };

// One target: the three 0-based source vertices and their area coordinates.  OUT_INSIDE / OUT_HULL: v, a are set.  OUT_FILL: the point is inside the convex hull
// but in a triangle of the completion (the reference throws).  OUT_LOST: beyond the hull and no hull edge faces it (a context without completion).
__device__ __forceinline__ int nodemap_weights_point(const InterpDev &d, double x, double y, int v[3], double a[3]) {
    long long dd[3] = {0, 0, 0}, Bx, By;
    const int it = locate(d, x, y, dd, Bx, By);
    if (it >= d.nels) return OUT_FILL;
    if (it >= 0) {
        const long long det = dd[0] + dd[1] + dd[2];   // == tb.det exactly
        a[0] = (double)dd[0] / det;                    // _weights.cpp:79-81
        a[1] = (double)dd[1] / det;
        a[2] = (double)dd[2] / det;
        v[0] = d.t0[it]; v[1] = d.t1[it]; v[2] = d.t2[it];
        return OUT_INSIDE;
    }
    // CloseBoundaryEdge (Mesh.cpp:4590-4627) on the convex hull, as k_interp reads it: the strip of the visible edge that holds the point, else the nearest hull
    // vertex.  The edge runs I = b -> J = a seen from outside; in the triangle behind it slot VerticesOfTriangularEdge[k][1] is I, [k][0] is J (_weights.cpp:105-107).
    int hit = -1, beste = -1, best_is_a = 0;
    double ha = 0., hb = 0.;
    long long bestd = 0x7fffffffffffffffll;
    for (int e = 0; e < d.nhull; ++e) {
        const HullDev h = d.hull[e];
        const long long ax = d.ix[h.a], ay = d.iy[h.a], bx = d.ix[h.b], by = d.iy[h.b];
        if (det3(ax, ay, bx, by, Bx, By) >= 0) continue;   // not visible from the point
        const long long IJx = ax - bx, IJy = ay - by;
        const long long IJ_IA = IJx * (Bx - bx) + IJy * (By - by), IJ_AJ = IJx * (ax - Bx) + IJy * (ay - By);
        if (IJ_IA >= 0 && IJ_AJ >= 0) {
            const double IJ2 = (double)(IJ_IA + IJ_AJ);
            hit = e; ha = IJ_AJ / IJ2; hb = IJ_IA / IJ2;
            break;
        }
        const long long da = (Bx - ax) * (Bx - ax) + (By - ay) * (By - ay), db = (Bx - bx) * (Bx - bx) + (By - by) * (By - by);
        if (da < bestd) { bestd = da; beste = e; best_is_a = 1; }
        if (db < bestd) { bestd = db; beste = e; best_is_a = 0; }
    }
    if (hit < 0) {
        if (beste < 0) return OUT_LOST;
        // the vertex outcome: a = 1, b = 0 at I or a = 0, b = 1 at J of a hull edge that ends there (Mesh.cpp:4611, 4616); which of the two edges the reference
        // stops on depends on its walk -- the weights are 1, 0, 0 either way
        hit = beste; ha = best_is_a ? 0. : 1.; hb = best_is_a ? 1. : 0.;
    }
    const HullDev h = d.hull[hit];
    const int kI = (h.k + 2) % 3, kJ = (h.k + 1) % 3;   // VerticesOfTriangularEdge[k][1], [k][0]; OppositeVertex[k] = k
    const double rest = 1 - ha - hb;
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = q == kI ? ha : (q == kJ ? hb : rest);   // (selects: a[] stays in registers)
    v[0] = d.t0[h.tri]; v[1] = d.t1[h.tri]; v[2] = d.t2[h.tri];
    return OUT_HULL;
}

struct Weights {   // the six rows of a map, [N] each
    int *v0, *v1, *v2;
    double *a0, *a1, *a2;
};

// counts: [0] targets in a fill triangle, [1] the first of them (starts at INT_MAX), [2] targets beyond the hull, [3] targets nothing faces
__global__ void __launch_bounds__(256) k_nodemap_weights(InterpDev d, const double *__restrict__ xi, const double *__restrict__ yi, Weights w, int *counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.N_interp) return;
    int v[3] = {0, 0, 0};
    double a[3] = {0., 0., 0.};
    const int rc = nodemap_weights_point(d, xi[i], yi[i], v, a);
    if (rc == OUT_FILL) { atomicAdd(counts, 1); atomicMin(counts + 1, i); }
    else if (rc == OUT_LOST) atomicAdd(counts + 3, 1);
    else if (rc == OUT_HULL) atomicAdd(counts + 2, 1);
    w.v0[i] = v[0]; w.v1[i] = v[1]; w.v2[i] = v[2];
    w.a0[i] = a[0]; w.a1[i] = a[1]; w.a2[i] = a[2];
}

struct SourceArgs {
    const double *field[kMaxVar];   // [G] each, as OASIS3::get_2d delivers them
    double a[kMaxVar], b[kMaxVar];
    int n_var, R;
    const int *reduced;             // [R] grid.reduced_nodes_ind, NULL = the identity
    int npairs, j0[kMaxPairs], j1[kMaxPairs];
    int east_west;                  // the pairs are east / north components (wave_cpl_nodes)
    const double *lat, *lon;        // [R] degrees, read only under east_west
    nxs_mapx_polar map;
    double Re;                      // mapx_Re_km*1000.
    int rotate;                     // ROTATE_*
    double c, s;                    // ROTATE_UNIFORM: cos / sin(-rotation_angle)
    const double *cs, *sn;          // ROTATE_GRID_THETA: [R] cos / sin(rotation - theta[i])
    double *stage;                  // [n_var][R] loaded_data
};

__global__ void __launch_bounds__(256) k_nodemap_source(SourceArgs s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.R) return;
    const int g = s.reduced ? s.reduced[i] : i;
    const size_t R = (size_t)s.R;
#pragma unroll
    for (int v = 0; v < kMaxVar; ++v)
        if (v < s.n_var) {
            double t = s.field[v][g];   // externaldata.cpp:498-509
            t *= s.a[v];
            t += s.b[v];
            s.stage[v * R + i] = t;
        }
#pragma unroll
    for (int k = 0; k < kMaxPairs; ++k)
        if (k < s.npairs) {
            double *p0 = s.stage + s.j0[k] * R + i, *p1 = s.stage + s.j1[k] * R + i;
            if (s.east_west) nf_east_north_point(s.map, s.Re, s.lat[i], s.lon[i], p0, p1);
            if (s.rotate != ROTATE_NONE) {
                const double c = s.rotate == ROTATE_UNIFORM ? s.c : s.cs[i], sn = s.rotate == ROTATE_UNIFORM ? s.s : s.sn[i];
                const double t0 = *p0, t1 = *p1;
                *p0 = c * t0 + sn * t1;      // externaldata.cpp:1255-1256, 1275-1276
                *p1 = -sn * t0 + c * t1;
            }
        }
}

struct GatherArgs {
    const double *stage;            // [NV][R]
    int R, N, get;                  // get: store factor*x + bias (ExternalData::get), else x
    double *out[kMaxVar];           // [N] each
    double factor[kMaxVar], bias[kMaxVar];
};

template <int NV>
__global__ void __launch_bounds__(256) k_nodemap_gather(GatherArgs g, const int *__restrict__ v0, const int *__restrict__ v1, const int *__restrict__ v2,
                                                        const double *__restrict__ a0, const double *__restrict__ a1, const double *__restrict__ a2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.N) return;
    const int i0 = v0[i], i1 = v1[i], i2 = v2[i];
    const double w0 = a0[i], w1 = a1[i], w2 = a2[i];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double *d = g.stage + (size_t)v * g.R;
        const double x = w0 * d[i0] + w1 * d[i1] + w2 * d[i2];   // _apply.cpp:57-59
        g.out[v][i] = g.get ? g.factor[v] * x + g.bias[v] : x;
    }
}

}  // namespace nodemap
