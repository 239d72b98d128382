// nxs_interp.hip -- mesh-to-mesh interpolation at regrid as a HIP gather kernel (include/nxs_interp.h).
//
// Reference: contrib/bamg/src/InterpFromMeshToMesh2dx.cpp:17-179 (called at FE.cpp:3131-3139), which
// locates every target point by walking bamg's triangulation with EXACT integer predicates:
//   integer coordinates  Mesh::SetIntCoor  contrib/bamg/src/Mesh.cpp:3441-3468  (bbox grown by 5 %,
//                        coefIcoor = (2^30-1)/max extent, truncation)   and R2ToI2 Mesh.cpp:3688-3690
//   determinants         include/det.h:8-12 (64-bit)
//   area coordinates     det3[k]/det, InterpFromMeshToMesh2dx.cpp:113-116
// The same integers are used here, so a point inside the data mesh gets the reference's weights bit for
// bit whatever triangle search is used; the search itself is a uniform bucket grid over the integer plane
// (one thread per target point, candidates tested in ascending triangle number).
#include <hip/hip_runtime.h>

#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <future>
#include <map>
#include <memory>
#include <string>
#include <system_error>
#include <vector>

#include "nxs_dyn.h"
#include "nxs_guard.hpp"
#include "nxs_interp.h"
#include "nxs_hull.inl"
#include "nxs_drifters.hpp"
#include "nxs_angles.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// handler of every extern "C" function-try-block of this file (nxs_guard.hpp): status code + text, never an exception across the ABI
int entry_caught(const char *entry) noexcept {
    return nxs_guard::caught(entry, [](int code, const char *text) { (void)fail(code, "%s", text); });
}

// Where the time of the last regrid call of this thread went (nxs_interp_last_timing): [0] connectivity tables of the old mesh, [1] integer
// plane + bucket grid, [2] convex completion, [3] host -> device copies, [4] kernels (HIP events), [5] device -> host copies, [6] whole call; ms.
thread_local double g_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
struct Tick {
    int slot; std::chrono::steady_clock::time_point t0;
    explicit Tick(int s) : slot(s), t0(std::chrono::steady_clock::now()) {}
    ~Tick() { g_ms[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Every device operation of this file runs on a stream of its own (one per host thread, created on first use), never on the
// legacy default stream: a host that drives several GPUs from one process may be capturing a graph of the dynamics step on
// another thread, and legacy-stream work is refused while a capture is open.
hipStream_t S() {
    thread_local hipStream_t st = nullptr;
    thread_local int st_dev = -1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!st || st_dev != dev) {
        st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { st = nullptr; (void)hipGetLastError(); }
        st_dev = dev;
    }
    return st;
}
hipError_t copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, S());
    return e != hipSuccess ? e : hipStreamSynchronize(S());
}
hipError_t memset_sync(void *dst, int value, size_t bytes) {
    const hipError_t e = hipMemsetAsync(dst, value, bytes, S());
    return e != hipSuccess ? e : hipStreamSynchronize(S());
}

struct BEdge {  // a boundary edge as seen from its (inside) triangle
    int tri, k;  // triangle number, local edge index (vertices VOTE[k][0] -> VOTE[k][1])
};

struct HullDev { int a, b, tri, k; };  // nxs_hull::HullEdge

struct InterpDev {
    int nods, nels, N_data, N_interp, nodal;
    int nels_all;                  // nels + the fill triangles of bamg's convex completion (isdefault == 0 only), numbered behind the mesh's
    int nhull;                     // hull edges, counter-clockwise; 0 = no completion (then the nearest boundary edge stands in)
    const HullDev *hull;
    const int *t0, *t1, *t2;       // 0-based vertices
    const int *ix, *iy;            // integer coordinates of the data vertices
    int G, shift;                  // bucket grid: G x G cells of 2^shift integer units
    const int *cell_off, *cell_tri;
    int nbe;
    const BEdge *bedges;
    double coef, pminx, pminy;     // R2ToI2
    double xmin, xmax, ymin, ymax; // unexpanded bbox (isdefault test, InterpFromMeshToMesh2dx.cpp:93)
    int isdefault;
    double defaultvalue;
};

__device__ __forceinline__ long long det3(long long ax, long long ay, long long bx, long long by, long long cx, long long cy) {
    // include/det.h:8-12
    const long long bax = bx - ax, bay = by - ay, cax = cx - ax, cay = cy - ay;
    return bax * cay - bay * cax;
}

// Exact point location: R2ToI2 (Mesh.cpp:3688-3690: truncation of coefIcoor*(P - pmin)), then the candidates of
// the bucket in ascending triangle number.  Returns the triangle (dd = its three integer area coordinates) or
// -1 when the point is in no triangle of the data mesh; Bx/By = the integer point.
__device__ __forceinline__ int locate(const InterpDev &d, double x, double y, long long dd[3], long long &Bx, long long &By) {
    const double fx = d.coef * (x - d.pminx), fy = d.coef * (y - d.pminy);
    const bool in_plane = fx > -1. && fx < 1073741824. && fy > -1. && fy < 1073741824.;
    // (Icoor1) of a double: truncation; beyond the range of an int the x86 conversion the reference runs on yields INT_MIN.  A
    // point outside the integer plane (more than 5 % of the extent beyond the data mesh's bounding box) keeps its true integer
    // coordinates -- the hull projection below needs them
    const bool fits_x = fx > -2147483649. && fx < 2147483648., fits_y = fy > -2147483649. && fy < 2147483648.;
    Bx = fits_x ? (long long)(int)fx : -2147483648ll;
    By = fits_y ? (long long)(int)fy : -2147483648ll;
    if (in_plane && Bx >= 0 && By >= 0) {
        const int cx = (int)(Bx >> d.shift), cy = (int)(By >> d.shift);
        if (cx < d.G && cy < d.G) {
            const int c = cy * d.G + cx;
            for (int q = d.cell_off[c]; q < d.cell_off[c + 1]; ++q) {
                const int t = d.cell_tri[q];
                const int v0 = d.t0[t], v1 = d.t1[t], v2 = d.t2[t];
                const long long x0 = d.ix[v0], y0 = d.iy[v0], x1 = d.ix[v1], y1 = d.iy[v1], x2 = d.ix[v2], y2 = d.iy[v2];
                const long long e0 = det3(x1, y1, x2, y2, Bx, By);  // area coordinate of vertex 0
                const long long e1 = det3(x2, y2, x0, y0, Bx, By);
                const long long e2 = det3(x0, y0, x1, y1, Bx, By);
                if (e0 >= 0 && e1 >= 0 && e2 >= 0 && (e0 + e1 + e2) > 0) { dd[0] = e0; dd[1] = e1; dd[2] = e2; return t; }
            }
        }
    }
    return -1;
}

// counters of one call: [0] points in no triangle of the data mesh, [1] of those, interpolated inside a fill triangle,
// [2] projected on the hull (CloseBoundaryEdge), [3] handled by the nearest-boundary-edge stand-in
__global__ void __launch_bounds__(256) k_interp(InterpDev d, const double *__restrict__ data, const double *__restrict__ xi,
                                                const double *__restrict__ yi, double *__restrict__ out, int *num_exterior) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.N_interp) return;
    const double x = xi[i], y = yi[i];
    double *o = out + (size_t)i * d.N_data;
    if (d.isdefault && (x < d.xmin || x > d.xmax || y < d.ymin || y > d.ymax)) {
        for (int j = 0; j < d.N_data; ++j) o[j] = d.defaultvalue;
        return;
    }
    long long dd[3] = {0, 0, 0}, Bx, By;
    int it = locate(d, x, y, dd, Bx, By);
    double a[3];
    if (it >= d.nels) {  // inside the hull, outside the mesh: a fill triangle of bamg's reconstructed mesh (Mesh.cpp:3135-3440)
        atomicAdd(num_exterior, 1);
        if (d.isdefault) {   // InterpFromMeshToMesh2dx.cpp:124-128 (reft < 0)
            for (int j = 0; j < d.N_data; ++j) o[j] = d.defaultvalue;
            return;
        }
        if (d.nodal) atomicAdd(num_exterior + 1, 1);
        else it = -2;        // element data: the reference stops with "Triangle number ... not in [0 nels]"; nearest boundary edge here
    }
    if (it >= 0) {
        const long long det = dd[0] + dd[1] + dd[2];  // == det(v0,v1,v2) exactly
        a[0] = (double)dd[0] / det;                   // InterpFromMeshToMesh2dx.cpp:113-116
        a[1] = (double)dd[1] / det;
        a[2] = (double)dd[2] / det;
    } else {
        if (d.isdefault) {
            for (int j = 0; j < d.N_data; ++j) o[j] = d.defaultvalue;
            return;
        }
        if (it == -1) atomicAdd(num_exterior, 1);
        const int VOTE[3][2] = {{1, 2}, {2, 0}, {0, 1}};
        // Beyond the hull: CloseBoundaryEdge (Mesh.cpp:4590-4627) slides along the hull edges until the point projects inside one
        // (a = IJ.AJ / IJ2 for I, b = IJ.IA / IJ2 for J, placed in the slots of the triangle behind that edge,
        // InterpFromMeshToMesh2dx.cpp:137-147) or changes direction at a vertex (weight 1 there).  On a convex hull the outward
        // strips of the edges and the cones of the vertices tile the outside, so the edge or vertex it stops at does not depend on
        // where it starts: the strip of a VISIBLE edge that holds the point, else the nearest hull vertex.
        if (it == -1 && d.nhull > 0 && d.nodal) {
            int hit = -1;
            double ha = 0., hb = 0.;
            long long bestd = 0x7fffffffffffffffll;
            int bestv = -1;
            for (int e = 0; e < d.nhull; ++e) {
                const HullDev h = d.hull[e];
                const long long ax = d.ix[h.a], ay = d.iy[h.a], bx = d.ix[h.b], by = d.iy[h.b];
                if (det3(ax, ay, bx, by, Bx, By) >= 0) continue;  // not visible from the point
                // seen from outside the edge runs I = b -> J = a
                const long long IJx = ax - bx, IJy = ay - by;
                const long long IJ_IA = IJx * (Bx - bx) + IJy * (By - by), IJ_AJ = IJx * (ax - Bx) + IJy * (ay - By);
                if (IJ_IA >= 0 && IJ_AJ >= 0) {
                    const double IJ2 = (double)(IJ_IA + IJ_AJ);
                    hit = e; ha = IJ_AJ / IJ2; hb = IJ_IA / IJ2;
                    break;
                }
                const long long da = (Bx - ax) * (Bx - ax) + (By - ay) * (By - ay), db = (Bx - bx) * (Bx - bx) + (By - by) * (By - by);
                if (da < bestd) { bestd = da; bestv = h.a; }
                if (db < bestd) { bestd = db; bestv = h.b; }
            }
            if (hit >= 0) {
                atomicAdd(num_exterior + 2, 1);
                const HullDev h = d.hull[hit];
                const int tv[3] = {d.t0[h.tri], d.t1[h.tri], d.t2[h.tri]};
                // in the triangle behind the edge: VOTE[k][1] is I = b, VOTE[k][0] is J = a
                a[VOTE[h.k][1]] = ha;
                a[VOTE[h.k][0]] = hb;
                a[h.k] = 1 - ha - hb;
                for (int j = 0; j < d.N_data; ++j)
                    o[j] = a[0] * data[(size_t)d.N_data * tv[0] + j] + a[1] * data[(size_t)d.N_data * tv[1] + j] + a[2] * data[(size_t)d.N_data * tv[2] + j];
                return;
            }
            if (bestv >= 0) {  // a = 1, b = 0 at a hull vertex: 1 * data + 0 * data + 0 * data
                atomicAdd(num_exterior + 2, 1);
                for (int j = 0; j < d.N_data; ++j) o[j] = data[(size_t)d.N_data * bestv + j];
                return;
            }
        }
        // stand-in (no completion for this mesh, or element data): nearest boundary edge, a/b as CloseBoundaryEdge
        atomicAdd(num_exterior + 3, 1);
        double best = INFINITY;
        int bk = -1;
        double ba = 0., bb = 0.;
        for (int e = 0; e < d.nbe; ++e) {
            const BEdge be = d.bedges[e];
            const int tv[3] = {d.t0[be.tri], d.t1[be.tri], d.t2[be.tri]};
            // seen from OUTSIDE the edge runs from the triangle's VOTE[k][1] to VOTE[k][0]
            const int vI = tv[VOTE[be.k][1]], vJ = tv[VOTE[be.k][0]];
            const long long Ix = d.ix[vI], Iy = d.iy[vI], Jx = d.ix[vJ], Jy = d.iy[vJ];
            const long long IJx = Jx - Ix, IJy = Jy - Iy;
            const long long IJ_IA = IJx * (Bx - Ix) + IJy * (By - Iy);
            const long long IJ_AJ = IJx * (Jx - Bx) + IJy * (Jy - By);
            double aa, b2, dist;
            if (IJ_IA < 0) { aa = 1.; b2 = 0.; dist = hypot((double)(Bx - Ix), (double)(By - Iy)); }
            else if (IJ_AJ < 0) { aa = 0.; b2 = 1.; dist = hypot((double)(Bx - Jx), (double)(By - Jy)); }
            else {
                const double IJ2 = (double)(IJ_IA + IJ_AJ);
                aa = IJ_AJ / IJ2;
                b2 = IJ_IA / IJ2;
                const double cr = (double)(IJx * (By - Iy) - IJy * (Bx - Ix));
                dist = fabs(cr) / sqrt(IJ2);
            }
            if (dist < best) { best = dist; bk = e; ba = aa; bb = b2; }
        }
        if (bk < 0) { for (int j = 0; j < d.N_data; ++j) o[j] = d.defaultvalue; return; }
        const BEdge be = d.bedges[bk];
        it = be.tri;
        // InterpFromMeshToMesh2dx.cpp:141-143, expressed in the inside triangle's local numbering
        a[VOTE[be.k][1]] = ba;
        a[VOTE[be.k][0]] = bb;
        a[be.k] = 1 - ba - bb;
    }
    if (d.nodal) {
        const int i0 = d.t0[it], i1 = d.t1[it], i2 = d.t2[it];
        for (int j = 0; j < d.N_data; ++j)  // InterpFromMeshToMesh2dx.cpp:151-156
            o[j] = a[0] * data[(size_t)d.N_data * i0 + j] + a[1] * data[(size_t)d.N_data * i1 + j] + a[2] * data[(size_t)d.N_data * i2 + j];
    } else {
        for (int j = 0; j < d.N_data; ++j) o[j] = data[(size_t)d.N_data * it + j];
    }
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) {   // (a buffer that is allocated again lets go of what it held)
        if (p) { (void)hipFree(p); p = nullptr; }
        return hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)) == hipSuccess ? 0 : -1;
    }
    int upload(const T *src, size_t n) {
        Tick tk(3);
        if (alloc(n)) return -1;
        return (n == 0 || copy_sync(p, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess) ? 0 : -1;
    }
};

}  // namespace

#include "nxs_regrid_tables.inl"

namespace {

struct GridDev {
    int nods, nels, N_data, nrows, ncols, nodal;
    const int *t0, *t1, *t2;
    const double *x, *y;
    const double *xg, *yg;  // grid coordinates as the reference builds them (InterpFromMeshToGridx.cpp:73-92)
    int G; double bx0, by0, bdx, bdy;  // bucket grid over the mesh bbox
    const int *cell_off, *cell_tri;
    double default_value;
};

// one thread per grid point; candidates in ascending element number, the LAST hit wins (the reference's
// element loop overwrites, InterpFromMeshToGridx.cpp:96-181)
__global__ void __launch_bounds__(256) k_mesh_to_grid(GridDev d, const double *__restrict__ data, double *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)d.nrows * d.ncols) return;
    const int i = (int)(gid / d.ncols), j = (int)(gid % d.ncols);
    const double xg = d.xg[i], yg = d.yg[j];
    double *o = out + (size_t)d.N_data * gid;
    for (int k = 0; k < d.N_data; ++k) o[k] = d.default_value;
    const int cx = (int)floor((xg - d.bx0) / d.bdx), cy = (int)floor((yg - d.by0) / d.bdy);
    if (cx < 0 || cy < 0 || cx >= d.G || cy >= d.G) return;
    const int c = cy * d.G + cx;
    int hit = -1;
    double h1 = 0., h2 = 0., h3 = 0.;
    for (int q = d.cell_off[c]; q < d.cell_off[c + 1]; ++q) {
        const int n = d.cell_tri[q];
        const int a = d.t0[n], b = d.t1[n], c3 = d.t2[n];
        const double x1 = d.x[a], y1 = d.y[a], x2 = d.x[b], y2 = d.y[b], x3 = d.x[c3], y3 = d.y[c3];
        double xmin = x1, xmax = x1, ymin = y1, ymax = y1;
        if (x2 < xmin) xmin = x2; if (x2 > xmax) xmax = x2; if (y2 < ymin) ymin = y2; if (y2 > ymax) ymax = y2;
        if (x3 < xmin) xmin = x3; if (x3 > xmax) xmax = x3; if (y3 < ymin) ymin = y3; if (y3 > ymax) ymax = y3;
        if ((xg > xmax) || (xg < xmin) || (yg > ymax) || (yg < ymin)) continue;  // :143, :148
        const double area = x2 * y3 - y2 * x3 + x1 * y2 - y1 * x2 + x3 * y1 - y3 * x1;  // :135-137
        const double area_1 = ((xg - x3) * (y2 - y3) - (yg - y3) * (x2 - x3)) / area;     // :152-153
        const double area_2 = ((x1 - x3) * (yg - y3) - (y1 - y3) * (xg - x3)) / area;     // :155-156
        const double area_3 = 1 - area_1 - area_2;
        if (area_1 > -10e-12 && area_2 > -10e-12 && area_3 > -10e-12) { hit = n; h1 = area_1; h2 = area_2; h3 = area_3; }
    }
    if (hit < 0) return;
    for (int k = 0; k < d.N_data; ++k) {
        double v;
        if (d.nodal) {
            v = h1 * data[(size_t)d.N_data * d.t0[hit] + k];
            v += h2 * data[(size_t)d.N_data * d.t1[hit] + k];
            v += h3 * data[(size_t)d.N_data * d.t2[hit] + k];
        } else {
            v = data[(size_t)d.N_data * hit + k];
        }
        if (isnan(v)) v = d.default_value;
        o[k] = v;
    }
}

}  // namespace

namespace {

// [n][3] triangles (1-based when `one_based`) -> three 0-based arrays
__global__ void __launch_bounds__(256) k_split_triangles(int n, const int *__restrict__ tri3, int one_based, int *__restrict__ t0, int *__restrict__ t1, int *__restrict__ t2) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    t0[e] = tri3[3 * e] - one_based; t1[e] = tri3[3 * e + 1] - one_based; t2[e] = tri3[3 * e + 2] - one_based;
}

__global__ void __launch_bounds__(256) k_add_int(int n, int *__restrict__ a, int c) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] += c;
}

// The data mesh in bamg's integer plane + the bucket grid used by locate(), resident on the device.
thread_local int g_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // of the last mesh-to-mesh call of this thread (nxs_interp_last_info)
thread_local std::string g_completion_note;

struct Locator {
    InterpDev d{};
    DevBuf<int> dtri3, dt0, dt1, dt2, dix, diy, doff, dtri;
    DevBuf<BEdge> dbe;
    DevBuf<HullDev> dhull;
    std::vector<int> ix, iy;      // host copies of the integer plane (the completion is host code)
    nxs_hull::Completion comp;
    bool with_completion = false;
    int nods = 0, nels_mesh = 0;
    double coef = 0., pminx = 0., pminy = 0.;

    // the data mesh in bamg's integer plane + the bucket grid of locate(), the grid built on the device (nxs_regrid_tables.inl)
    int build(const int32_t *index_data, const double *x_data, const double *y_data, int32_t nods_, int32_t nels, bool need_boundary_edges,
              const nxs_hull::Completion *ready = nullptr) {
        nods = nods_; nels_mesh = nels;
        {   // ---- SetIntCoor (Mesh.cpp:3441-3468)
            Tick tk(1);
            double bx0 = x_data[0], by0 = y_data[0], bx1 = x_data[0], by1 = y_data[0];
            for (int i = 0; i < nods; ++i) {
                bx0 = std::min(bx0, x_data[i]); by0 = std::min(by0, y_data[i]);
                bx1 = std::max(bx1, x_data[i]); by1 = std::max(by1, y_data[i]);
            }
            d.xmin = bx0; d.xmax = bx1; d.ymin = by0; d.ymax = by1;
            if (!nxs_hull::int_plane(x_data, y_data, nods, ix, iy, coef, pminx, pminy))
                return fail(NXS_ERR_INVALID, "coefIcoor should be positive, a problem in the geometry is likely");
        }
        // ---- bamg's convex completion (isdefault == 0 only): fill triangles numbered behind the mesh's, hull edges
        std::vector<HullDev> hull;
        std::vector<int> fill3;  // AoS, 0-based
        if (need_boundary_edges) {
            Tick tk(2);
            comp = ready ? *ready : nxs_hull::complete_any(index_data, ix.data(), iy.data(), nods, nels);
            with_completion = true;
            if (comp.ok) {
                fill3 = comp.fill;
                for (const auto &h : comp.hull) hull.push_back(HullDev{h.a, h.b, h.tri, h.k});
            }
        }
        const int nfill = (int)fill3.size() / 3, nall = nels + nfill;
        // ---- boundary edges (edges held by exactly one triangle): the stand-in for exterior points when no completion exists
        std::vector<BEdge> bedges;
        if (need_boundary_edges && !comp.ok) {
            Tick tk(2);
            std::vector<int> bnd;
            (void)nxs_hull::find_boundary_edges(index_data, nods, nels, bnd);
            for (int be : bnd) bedges.push_back(BEdge{be / 3, be % 3});
        }
        // ---- triangles to the device (1-based AoS as the caller has them), SoA 0-based there; the fill triangles behind them
        if (dtri3.alloc(3 * (size_t)nall) || dt0.alloc(nall) || dt1.alloc(nall) || dt2.alloc(nall))
            return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        {
            Tick tk(3);
            if (copy_sync(dtri3.p, index_data, 3 * (size_t)nels * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
        }
        hipLaunchKernelGGL(k_split_triangles, dim3((nels + 255) / 256), dim3(256), 0, S(), nels, dtri3.p, 1, dt0.p, dt1.p, dt2.p);
        if (nfill > 0) {
            Tick tk(3);
            if (copy_sync(dtri3.p + 3 * (size_t)nels, fill3.data(), fill3.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
            hipLaunchKernelGGL(k_split_triangles, dim3((nfill + 255) / 256), dim3(256), 0, S(), nfill, dtri3.p + 3 * (size_t)nels, 0, dt0.p + nels, dt1.p + nels, dt2.p + nels);
        }
        if (dix.upload(ix.data(), nods) || diy.upload(iy.data(), nods) || dbe.upload(bedges.data(), bedges.size()) || dhull.upload(hull.data(), hull.size()))
            return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
        // ---- bucket grid over the integer plane, on the device: count -> scan -> fill -> sort every cell's list ascending
        int G = 1;
        while ((long long)G * G * 2 < nall && G < 4096) G <<= 1;
        int shift = 30;
        for (int g = G; g > 1; g >>= 1) --shift;  // cell = 2^shift units, G cells cover [0, 2^30)
        const size_t ncell = (size_t)G * G;
        DevBuf<int> cursor, wide, nwide;
        if (doff.alloc(ncell + 1) || cursor.alloc(ncell) || wide.alloc(nall) || nwide.alloc(1)) return fail(NXS_ERR_HIP, "device allocation failed");
        int total = 0, n_wide = 0;
        {
            Tick tk(1);
            if (hipMemsetAsync(doff.p, 0, (ncell + 1) * sizeof(int), S()) != hipSuccess || hipMemsetAsync(cursor.p, 0, ncell * sizeof(int), S()) != hipSuccess ||
                hipMemsetAsync(nwide.p, 0, sizeof(int), S()) != hipSuccess)
                return fail(NXS_ERR_HIP, "hipMemset failed");
            hipLaunchKernelGGL(regrid_tables::k_grid_count, dim3((nall + 255) / 256), dim3(256), 0, S(), nall, (const int *)dt0.p, (const int *)dt1.p, (const int *)dt2.p,
                               (const int *)dix.p, (const int *)diy.p, shift, G, doff.p, wide.p, nwide.p);
            if (copy_sync(&n_wide, nwide.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
            if (n_wide > 0)  // triangles that span many cells (fill triangles across a bay): a workgroup each
                hipLaunchKernelGGL(regrid_tables::k_grid_count_wide, dim3(n_wide), dim3(256), 0, S(), (const int *)wide.p, (const int *)dt0.p, (const int *)dt1.p, (const int *)dt2.p,
                                   (const int *)dix.p, (const int *)diy.p, shift, G, doff.p);
            if (regrid_tables::exclusive_scan(doff.p, (int)(ncell + 1), S()) != hipSuccess) return fail(NXS_ERR_HIP, "scan of the bucket grid failed");
            if (copy_sync(&total, doff.p + ncell, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
            if (dtri.alloc((size_t)std::max(total, 1))) return fail(NXS_ERR_HIP, "device allocation failed");
            hipLaunchKernelGGL(regrid_tables::k_grid_fill, dim3((nall + 255) / 256), dim3(256), 0, S(), nall, (const int *)dt0.p, (const int *)dt1.p, (const int *)dt2.p,
                               (const int *)dix.p, (const int *)diy.p, shift, G, (const int *)doff.p, cursor.p, dtri.p);
            if (n_wide > 0)
                hipLaunchKernelGGL(regrid_tables::k_grid_fill_wide, dim3(n_wide), dim3(256), 0, S(), (const int *)wide.p, (const int *)dt0.p, (const int *)dt1.p, (const int *)dt2.p,
                                   (const int *)dix.p, (const int *)diy.p, shift, G, (const int *)doff.p, cursor.p, dtri.p);
            hipLaunchKernelGGL(regrid_tables::k_rows_sort, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, S(), (int)ncell, (const int *)doff.p, dtri.p, 0);
            if (hipStreamSynchronize(S()) != hipSuccess) return fail(NXS_ERR_HIP, "bucket grid kernels failed: %s", hipGetErrorString(hipGetLastError()));
        }
        d.nods = nods; d.nels = nels; d.nels_all = nall;
        d.nhull = (int)hull.size(); d.hull = dhull.p;
        d.t0 = dt0.p; d.t1 = dt1.p; d.t2 = dt2.p; d.ix = dix.p; d.iy = diy.p;
        d.G = G; d.shift = shift; d.cell_off = doff.p; d.cell_tri = dtri.p;
        d.nbe = (int)bedges.size(); d.bedges = dbe.p;
        d.coef = coef; d.pminx = pminx; d.pminy = pminy;
        return 0;
    }
};

}  // namespace

namespace {
int mesh_to_grid(double *griddata, const int32_t *index_mesh, const double *x_mesh, const double *y_mesh,
                 int32_t nods, int32_t nels, const double *data_mesh, bool data_on_device, int32_t data_length, int32_t N_data,
                 double xmin, double ymax, double xposting, double yposting, int32_t nrows, int32_t ncols,
                 double default_value, int32_t device, double *kernel_ms) {
    if (!griddata || !index_mesh || !x_mesh || !y_mesh || !data_mesh) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nels < 1 || nods < 3 || ncols < 1 || nrows < 1 || xposting == 0 || yposting == 0 || N_data < 1)  // :34-36
        return fail(NXS_ERR_INVALID, "nothing to be done according to the mesh given in input");
    if (data_length != nods && data_length != nels)
        return fail(NXS_ERR_INVALID, "length of vector data not supported yet. It should be of length (number of nodes) or (number of elements)!");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the interpolation has no CPU path");
    if (device < 0 || device >= ndev) return fail(NXS_ERR_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    for (int64_t i = 0; i < 3ll * nels; ++i)
        if (index_mesh[i] < 1 || index_mesh[i] > nods) return fail(NXS_ERR_INVALID, "index_mesh[%lld] out of range", (long long)i);

    // grid coordinates exactly as the reference builds them (flips included), :66-92
    std::vector<double> xg(nrows), yg(ncols);
    if (xposting < 0) { for (int i = 0; i < nrows; ++i) xg[nrows - 1 - i] = xmin - xposting * i; }
    else { for (int i = 0; i < nrows; ++i) xg[i] = xmin + xposting * i; }
    if (yposting < 0) { for (int i = 0; i < ncols; ++i) yg[i] = ymax + yposting * i; }
    else { for (int i = 0; i < ncols; ++i) yg[ncols - 1 - i] = ymax - yposting * i; }

    std::vector<int> t0(nels), t1(nels), t2(nels);
    double bx0 = x_mesh[0], bx1 = x_mesh[0], by0 = y_mesh[0], by1 = y_mesh[0];
    for (int i = 0; i < nods; ++i) { bx0 = std::min(bx0, x_mesh[i]); bx1 = std::max(bx1, x_mesh[i]); by0 = std::min(by0, y_mesh[i]); by1 = std::max(by1, y_mesh[i]); }
    for (int e = 0; e < nels; ++e) { t0[e] = index_mesh[3 * e] - 1; t1[e] = index_mesh[3 * e + 1] - 1; t2[e] = index_mesh[3 * e + 2] - 1; }
    int G = 1;
    while ((long long)G * G * 2 < nels && G < 4096) G <<= 1;
    const double bdx = (bx1 - bx0) / G * (1. + 1e-12) + 1e-300, bdy = (by1 - by0) / G * (1. + 1e-12) + 1e-300;
    auto cellr = [&](int e, int &a, int &b, int &c, int &dd2) {
        const double xs[3] = {x_mesh[t0[e]], x_mesh[t1[e]], x_mesh[t2[e]]}, ys[3] = {y_mesh[t0[e]], y_mesh[t1[e]], y_mesh[t2[e]]};
        a = (int)std::floor((std::min({xs[0], xs[1], xs[2]}) - bx0) / bdx) - 1; b = (int)std::floor((std::max({xs[0], xs[1], xs[2]}) - bx0) / bdx) + 1;
        c = (int)std::floor((std::min({ys[0], ys[1], ys[2]}) - by0) / bdy) - 1; dd2 = (int)std::floor((std::max({ys[0], ys[1], ys[2]}) - by0) / bdy) + 1;
        a = std::max(a, 0); c = std::max(c, 0); b = std::min(b, G - 1); dd2 = std::min(dd2, G - 1);
    };
    std::vector<int> cnt((size_t)G * G + 1, 0);
    for (int e = 0; e < nels; ++e) { int a, b, c, dd2; cellr(e, a, b, c, dd2); for (int cy = c; cy <= dd2; ++cy) for (int cx = a; cx <= b; ++cx) cnt[(size_t)cy * G + cx + 1]++; }
    for (size_t c = 0; c < (size_t)G * G; ++c) cnt[c + 1] += cnt[c];
    std::vector<int> cell_tri(cnt[(size_t)G * G]), fill(cnt.begin(), cnt.end() - 1);
    for (int e = 0; e < nels; ++e) { int a, b, c, dd2; cellr(e, a, b, c, dd2); for (int cy = c; cy <= dd2; ++cy) for (int cx = a; cx <= b; ++cx) cell_tri[fill[(size_t)cy * G + cx]++] = e; }

    DevBuf<int> dt0, dt1, dt2, doff, dtri;
    DevBuf<double> dx, dy, dxg, dyg, ddata, dout;
    const size_t npts = (size_t)nrows * ncols;
    if (dt0.upload(t0.data(), nels) || dt1.upload(t1.data(), nels) || dt2.upload(t2.data(), nels) || doff.upload(cnt.data(), cnt.size()) ||
        dtri.upload(cell_tri.data(), cell_tri.size()) || dx.upload(x_mesh, nods) || dy.upload(y_mesh, nods) || dxg.upload(xg.data(), nrows) ||
        dyg.upload(yg.data(), ncols) || (!data_on_device && ddata.upload(data_mesh, (size_t)data_length * N_data)) || dout.alloc(npts * N_data))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    GridDev d{};
    d.nods = nods; d.nels = nels; d.N_data = N_data; d.nrows = nrows; d.ncols = ncols; d.nodal = (data_length == nods);
    d.t0 = dt0.p; d.t1 = dt1.p; d.t2 = dt2.p; d.x = dx.p; d.y = dy.p; d.xg = dxg.p; d.yg = dyg.p;
    d.G = G; d.bx0 = bx0; d.by0 = by0; d.bdx = bdx; d.bdy = bdy; d.cell_off = doff.p; d.cell_tri = dtri.p;
    d.default_value = default_value;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, S());
    hipLaunchKernelGGL(k_mesh_to_grid, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, S(), d, data_on_device ? data_mesh : (const double *)ddata.p, dout.p);
    (void)hipEventRecord(e1, S());
    hipError_t err = hipStreamSynchronize(S());
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(NXS_ERR_HIP, "mesh-to-grid kernel failed: %s", hipGetErrorString(err));
    if (kernel_ms) *kernel_ms = ms;
    if (copy_sync(griddata, dout.p, npts * N_data * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
}
}  // namespace

extern "C" int nxs_interp_mesh_to_grid(double *griddata, const int32_t *index_mesh, const double *x_mesh, const double *y_mesh,
                                       int32_t nods, int32_t nels, const double *data_mesh, int32_t data_length, int32_t N_data,
                                       double xmin, double ymax, double xposting, double yposting, int32_t nrows, int32_t ncols,
                                       double default_value, int32_t device, double *kernel_ms) try {
    return mesh_to_grid(griddata, index_mesh, x_mesh, y_mesh, nods, nels, data_mesh, false, data_length, N_data, xmin, ymax, xposting, yposting, nrows, ncols,
                        default_value, device, kernel_ms);
} catch (...) { return entry_caught("nxs_interp_mesh_to_grid"); }

// The same sampling with the mesh data ALREADY ON THE DEVICE (e.g. the rows of nxs_dyn_ice_diagnostics, or any [data_length][N_data] array of
// the caller's on `device`): a Moorings record (gridoutput.cpp:496) then needs no round trip of the element state through the host.  The caller
// makes sure the producer of data_mesh_device has finished (nxs_dyn_ice_diagnostics returns synchronised).
extern "C" int nxs_interp_mesh_to_grid_device(double *griddata, const int32_t *index_mesh, const double *x_mesh, const double *y_mesh,
                                              int32_t nods, int32_t nels, const double *data_mesh_device, int32_t data_length, int32_t N_data,
                                              double xmin, double ymax, double xposting, double yposting, int32_t nrows, int32_t ncols,
                                              double default_value, int32_t device, double *kernel_ms) try {
    return mesh_to_grid(griddata, index_mesh, x_mesh, y_mesh, nods, nels, data_mesh_device, true, data_length, N_data, xmin, ymax, xposting, yposting, nrows, ncols,
                        default_value, device, kernel_ms);
} catch (...) { return entry_caught("nxs_interp_mesh_to_grid_device"); }

extern "C" const char *nxs_interp_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------------------------------------
// A regrid's context: everything about the OLD mesh that both interpolation calls of FiniteElement::interpFields (FE.cpp:3071-3154: the
// conservative remapping of the element variables, then InterpFromMeshToMesh2dx of the nodal ones) and any later call on the same mesh need --
// the integer plane, the bucket grid, bamg's convex completion, the two connectivity tables -- built once, on the device where that is
// possible (nxs_regrid_tables.inl), and kept.  The one-shot entry points below make a context, use it and drop it.
// ---------------------------------------------------------------------------------------------------------
struct nxs_regrid {
    std::future<nxs_hull::Completion> completion;   // bamg's convex completion, started on a host thread when the context is made (it is pure
                                                    // host work on the context's own copies): ready by the time the nodal interpolation asks for it
    int device = 0;
    int32_t nods = 0, nels = 0;
    std::vector<int32_t> index;   // host copies (the completion is host code; the caller's arrays may go away)
    std::vector<double> x, y;
    Locator plain, full;          // without / with bamg's convex completion (isdefault != 0 / == 0)
    bool have_plain = false, have_full = false;
    DevBuf<int> dtrio, ddeg, dnec, dec;   // old triangles (AoS, 0-based), NodalElementConnectivity, ElementConnectivity as ints
    DevBuf<double> dxo, dyo;
    int nec_width = 0;
    bool have_conn = false;
};

namespace {

int regrid_locator(nxs_regrid *r, bool with_completion, Locator **out) {
    Locator &L = with_completion ? r->full : r->plain;
    bool &have = with_completion ? r->have_full : r->have_plain;
    if (!have) {
        nxs_hull::Completion ready;
        const bool use_ready = with_completion && r->completion.valid();
        if (use_ready) { Tick tk(2); ready = r->completion.get(); }   // (what is left to wait for, if anything)
        if (int rc = L.build(r->index.data(), r->x.data(), r->y.data(), r->nods, r->nels, with_completion, use_ready ? &ready : nullptr)) return rc;
        have = true;
    }
    *out = &L;
    return 0;
}

// the two tables checkTriangle walks, as ints (-1 = bamg's NaN): built on the device, or converted from the caller's bamg tables
int regrid_connectivity(nxs_regrid *r, const double *nec_old, int32_t nec_width, const double *ec_old) {
    if (r->have_conn && !nec_old && !ec_old) return 0;
    Tick tk(0);
    const int nods = r->nods, nels = r->nels;
    if (r->dtrio.p == nullptr) {
        if (r->dtrio.alloc(3 * (size_t)nels) || r->dxo.upload(r->x.data(), nods) || r->dyo.upload(r->y.data(), nods)) return fail(NXS_ERR_HIP, "device allocation / upload failed");
        if (copy_sync(r->dtrio.p, r->index.data(), 3 * (size_t)nels * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
        hipLaunchKernelGGL(k_add_int, dim3((3 * nels + 255) / 256), dim3(256), 0, S(), 3 * nels, r->dtrio.p, -1);
    }
    auto to_index = [&](double v, int hi) -> int {  // "(int)(v - 1)" of the reference; NaN and junk become "no more entries"
        if (!(v >= 1.) || !(v <= (double)hi)) return -1;
        return (int)v - 1;
    };
    if (nec_old) {  // bamgmesh_previous->NodalElementConnectivity as bamg left it
        if (nec_width < 1 || nec_width > 255) return fail(NXS_ERR_INVALID, "NodalElementConnectivity width %d (1 .. 255 expected)", nec_width);
        std::vector<int> neci((size_t)nods * nec_width);
        for (size_t i = 0; i < neci.size(); ++i) neci[i] = to_index(nec_old[i], nels);
        DevBuf<int> nb;
        if (nb.upload(neci.data(), neci.size())) return fail(NXS_ERR_HIP, "upload failed");
        std::swap(r->dnec.p, nb.p);
        r->nec_width = nec_width;
    } else if (!r->have_conn) {
        DevBuf<int> cursor, maxdeg;
        if (r->ddeg.alloc(nods) || cursor.alloc(nods) || maxdeg.alloc(1)) return fail(NXS_ERR_HIP, "device allocation failed");
        if (hipMemsetAsync(r->ddeg.p, 0, (size_t)nods * sizeof(int), S()) != hipSuccess || hipMemsetAsync(cursor.p, 0, (size_t)nods * sizeof(int), S()) != hipSuccess ||
            hipMemsetAsync(maxdeg.p, 0, sizeof(int), S()) != hipSuccess) return fail(NXS_ERR_HIP, "hipMemset failed");
        hipLaunchKernelGGL(regrid_tables::k_fan_count, dim3((3 * nels + 255) / 256), dim3(256), 0, S(), nels, (const int *)r->dtrio.p, r->ddeg.p, maxdeg.p);
        int w1 = 0;
        if (copy_sync(&w1, maxdeg.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
        if (w1 < 1 || w1 > 255) return fail(NXS_ERR_INVALID, "NodalElementConnectivity wider than 255 (%d)", w1);
        if (r->dnec.alloc((size_t)nods * w1)) return fail(NXS_ERR_HIP, "device allocation failed");
        hipLaunchKernelGGL(regrid_tables::k_fan_fill, dim3((3 * nels + 255) / 256), dim3(256), 0, S(), nels, (const int *)r->dtrio.p, cursor.p, r->dnec.p, w1);
        hipLaunchKernelGGL(regrid_tables::k_fan_sort_desc, dim3((nods + 255) / 256), dim3(256), 0, S(), nods, (const int *)r->ddeg.p, r->dnec.p, w1);
        if (hipStreamSynchronize(S()) != hipSuccess) return fail(NXS_ERR_HIP, "connectivity kernels failed: %s", hipGetErrorString(hipGetLastError()));
        r->nec_width = w1;
    }
    if (ec_old) {
        std::vector<int> eci(3 * (size_t)nels);
        for (size_t i = 0; i < eci.size(); ++i) eci[i] = to_index(ec_old[i], nels);
        DevBuf<int> eb;
        if (eb.upload(eci.data(), eci.size())) return fail(NXS_ERR_HIP, "upload failed");
        std::swap(r->dec.p, eb.p);
    } else if (!r->have_conn || nec_old) {
        // (from the ascending-independent fans: with the caller's NodalElementConnectivity the degrees are not known here, so the fans are rebuilt)
        DevBuf<int> deg2, cur2, nec2, maxdeg, bad;
        const int *deg = r->ddeg.p; const int *nec = r->dnec.p; int w = r->nec_width;
        if (nec_old) {
            if (deg2.alloc(nods) || cur2.alloc(nods) || maxdeg.alloc(1)) return fail(NXS_ERR_HIP, "device allocation failed");
            if (hipMemsetAsync(deg2.p, 0, (size_t)nods * sizeof(int), S()) != hipSuccess || hipMemsetAsync(cur2.p, 0, (size_t)nods * sizeof(int), S()) != hipSuccess ||
                hipMemsetAsync(maxdeg.p, 0, sizeof(int), S()) != hipSuccess) return fail(NXS_ERR_HIP, "hipMemset failed");
            hipLaunchKernelGGL(regrid_tables::k_fan_count, dim3((3 * nels + 255) / 256), dim3(256), 0, S(), nels, (const int *)r->dtrio.p, deg2.p, maxdeg.p);
            int w1 = 0;
            if (copy_sync(&w1, maxdeg.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
            if (nec2.alloc((size_t)nods * std::max(w1, 1))) return fail(NXS_ERR_HIP, "device allocation failed");
            hipLaunchKernelGGL(regrid_tables::k_fan_fill, dim3((3 * nels + 255) / 256), dim3(256), 0, S(), nels, (const int *)r->dtrio.p, cur2.p, nec2.p, w1);
            deg = deg2.p; nec = nec2.p; w = w1;
        }
        if (bad.alloc(1) || hipMemsetAsync(bad.p, 0, sizeof(int), S()) != hipSuccess) return fail(NXS_ERR_HIP, "device allocation failed");
        if (r->dec.p == nullptr && r->dec.alloc(3 * (size_t)nels)) return fail(NXS_ERR_HIP, "device allocation failed");
        hipLaunchKernelGGL(regrid_tables::k_elem_conn, dim3((3 * nels + 255) / 256), dim3(256), 0, S(), nels, (const int *)r->dtrio.p, deg, nec, w, r->dec.p, bad.p);
        int nbad = 0;
        if (copy_sync(&nbad, bad.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
        if (nbad > 0) return fail(NXS_ERR_INVALID, "an edge of the old mesh is shared by more than two triangles");
    }
    r->have_conn = !nec_old && !ec_old;   // (tables converted from the caller's are not kept for a later call without them)
    return 0;
}

}  // namespace

namespace {
// want_completion == false: the context of a one-shot call that will never look outside the mesh (the conservative remapping, the nodal interpolation
// with a default value): no completion thread is started -- nxs_regrid_destroy would only wait for work nobody asked for
int regrid_create(const int32_t *index_old, const double *x_old, const double *y_old, int32_t nods_old, int32_t nels_old, int32_t device,
                  nxs_regrid **out, bool want_completion) {
    if (!out) return fail(NXS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!index_old || !x_old || !y_old) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nods_old < 3 || nels_old < 1) return fail(NXS_ERR_INVALID, "bad sizes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the regrid interpolation has no CPU path");
    if (device < 0 || device >= ndev) return fail(NXS_ERR_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    for (int64_t i = 0; i < 3ll * nels_old; ++i)
        if (index_old[i] < 1 || index_old[i] > nods_old) return fail(NXS_ERR_INVALID, "index_old[%lld] out of range", (long long)i);
    std::unique_ptr<nxs_regrid> r(new nxs_regrid());
    r->device = device; r->nods = nods_old; r->nels = nels_old;
    r->index.assign(index_old, index_old + 3 * (size_t)nels_old);
    r->x.assign(x_old, x_old + nods_old); r->y.assign(y_old, y_old + nods_old);
    // The two connectivity tables are built on the device right away (2 ms at 1.5 M triangles): the conservative remapping walks them, and the
    // boundary edges bamg's convex completion starts from are the entries of ElementConnectivity without a neighbour -- a few thousand numbers to
    // copy back instead of a host pass over every triangle.  A mesh the device tables cannot describe (an edge in three triangles, inconsistent
    // orientation) is left to the host code, which says what is wrong with it when the completion is asked for.
    std::vector<int> bnd;
    bool have_bnd = false;
    if (regrid_connectivity(r.get(), nullptr, 0, nullptr) == 0) {
        DevBuf<int> cnt, list;
        const int cap = 3 * nels_old;
        if (!cnt.alloc(2) && !list.alloc((size_t)cap) && hipMemsetAsync(cnt.p, 0, 2 * sizeof(int), S()) == hipSuccess) {
            hipLaunchKernelGGL(regrid_tables::k_boundary_list, dim3((3 * nels_old + 255) / 256), dim3(256), 0, S(), nels_old, (const int *)r->dtrio.p, (const int *)r->dec.p,
                               cnt.p, list.p, cap, cnt.p + 1);
            int c2[2] = {0, 0};
            if (copy_sync(c2, cnt.p, sizeof c2, hipMemcpyDeviceToHost) == hipSuccess && c2[1] == 0 && c2[0] >= 0 && c2[0] <= cap) {
                bnd.resize((size_t)c2[0]);
                if (c2[0] == 0 || copy_sync(bnd.data(), list.p, bnd.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
                    std::sort(bnd.begin(), bnd.end());
                    have_bnd = true;
                }
            }
        }
    } else {
        (void)hipGetLastError();
        g_err.clear();   // (not this call's failure: the remapping reports it if it is asked for)
    }
    if (want_completion) try {   // bamg's convex completion on a host thread, from now on (pure host work on this context's own copies); without a thread it is made when asked for
        nxs_regrid *q = r.get();
        r->completion = std::async(std::launch::async, [q, have_bnd, bnd = std::move(bnd)]() {
            std::vector<int> ix, iy;
            double coef = 0., px = 0., py = 0.;
            if (!nxs_hull::int_plane(q->x.data(), q->y.data(), q->nods, ix, iy, coef, px, py)) { nxs_hull::Completion c; c.why = "coefIcoor should be positive"; return c; }
            return nxs_hull::complete_any(q->index.data(), ix.data(), iy.data(), q->nods, q->nels, 0, have_bnd ? &bnd : nullptr);
        });
    } catch (const std::system_error &) { }
    *out = r.release();
    return NXS_OK;
}
}  // namespace

extern "C" int nxs_regrid_create(const int32_t *index_old, const double *x_old, const double *y_old, int32_t nods_old, int32_t nels_old, int32_t device,
                                 nxs_regrid **out) try {
    return regrid_create(index_old, x_old, y_old, nods_old, nels_old, device, out, true);
} catch (...) { return entry_caught("nxs_regrid_create"); }

extern "C" int nxs_regrid_destroy(nxs_regrid *r) try {
    if (!r) return NXS_OK;
    (void)hipSetDevice(r->device);
    if (r->completion.valid()) { try { (void)r->completion.get(); } catch (...) { } }   // the thread reads this context: it ends before the context does
    delete r;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_regrid_destroy"); }

// InterpFromMeshToMesh2dx on the context's mesh.  flags: NXS_REGRID_IN_DEVICE = `data` is a device pointer, NXS_REGRID_OUT_DEVICE = `data_interp` is.
extern "C" int nxs_regrid_interp_nodes(nxs_regrid *r, double *data_interp, const double *data, int32_t M_data, int32_t N_data, const double *x_interp,
                                       const double *y_interp, int32_t N_interp, int32_t isdefault, double defaultvalue, int32_t flags,
                                       int32_t *num_exterior, double *kernel_ms) try {
    if (!r || !data_interp || !data || !x_interp || !y_interp) return fail(NXS_ERR_INVALID, "NULL argument");
    if (N_data <= 0 || N_interp < 0) return fail(NXS_ERR_INVALID, "bad sizes");
    const int nods = r->nods, nels = r->nels;
    if (M_data != nods && M_data != nels)  // InterpFromMeshToMesh2dx.cpp:39-42
        return fail(NXS_ERR_INVALID, "data provided should have either %d or %d lines (not %d)", nods, nels, M_data);
    if (hipSetDevice(r->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    for (double &v : g_ms) v = 0.;
    Tick whole(6);
    Locator *locp = nullptr;
    if (int rc = regrid_locator(r, !isdefault, &locp)) return rc;
    Locator &loc = *locp;
    InterpDev d = loc.d;
    DevBuf<int> dnext;
    DevBuf<double> ddata, dxi, dyi, dout;
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    if ((!in_dev && ddata.upload(data, (size_t)M_data * N_data)) || dxi.upload(x_interp, N_interp) || dyi.upload(y_interp, N_interp) ||
        (!out_dev && dout.alloc((size_t)N_interp * N_data)) || dnext.alloc(4))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    if (memset_sync(dnext.p, 0, 4 * sizeof(int)) != hipSuccess) return fail(NXS_ERR_HIP, "hipMemset failed");
    d.N_data = N_data; d.N_interp = N_interp; d.nodal = (M_data == nods);
    d.isdefault = isdefault != 0; d.defaultvalue = defaultvalue;
    double *outp = out_dev ? data_interp : dout.p;

    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, S());
    if (N_interp > 0)
        hipLaunchKernelGGL(k_interp, dim3((N_interp + 255) / 256), dim3(256), 0, S(), d, in_dev ? data : (const double *)ddata.p, (const double *)dxi.p,
                           (const double *)dyi.p, outp, dnext.p);
    (void)hipEventRecord(e1, S());
    hipError_t err = hipStreamSynchronize(S());
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(NXS_ERR_HIP, "interpolation kernel failed: %s", hipGetErrorString(err));
    g_ms[4] += ms;
    if (kernel_ms) *kernel_ms = ms;
    {
        Tick tk(5);
        if (!out_dev && N_interp > 0 && copy_sync(data_interp, dout.p, (size_t)N_interp * N_data * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(NXS_ERR_HIP, "copy back failed");
    }
    int next[4] = {0, 0, 0, 0};
    (void)copy_sync(next, dnext.p, sizeof next, hipMemcpyDeviceToHost);
    if (num_exterior) *num_exterior = next[0];
    g_info[0] = (int)loc.comp.fill.size() / 3; g_info[1] = (int)loc.comp.hull.size();
    g_info[2] = next[0]; g_info[3] = next[1]; g_info[4] = next[2]; g_info[5] = next[3];
    g_info[6] = (!isdefault && !loc.comp.ok) ? 1 : 0;
    g_completion_note = loc.comp.ok ? "" : loc.comp.why;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_regrid_interp_nodes"); }

extern "C" int nxs_interp_mesh_to_mesh_2d(double *data_interp, const int32_t *index_data, const double *x_data,
                                          const double *y_data, int32_t nods, int32_t nels, const double *data, int32_t M_data,
                                          int32_t N_data, const double *x_interp, const double *y_interp, int32_t N_interp,
                                          int32_t isdefault, double defaultvalue, int32_t device, int32_t *num_exterior,
                                          double *kernel_ms) try {
    if (!data_interp || !index_data || !x_data || !y_data || !data || !x_interp || !y_interp) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nods <= 0 || nels <= 0 || N_data <= 0 || N_interp < 0) return fail(NXS_ERR_INVALID, "bad sizes");
    if (M_data != nods && M_data != nels)  // InterpFromMeshToMesh2dx.cpp:39-42
        return fail(NXS_ERR_INVALID, "data provided should have either %d or %d lines (not %d)", nods, nels, M_data);
    nxs_regrid *r = nullptr;
    if (int rc = regrid_create(index_data, x_data, y_data, nods, nels, device, &r, isdefault == 0)) return rc;
    const int rc = nxs_regrid_interp_nodes(r, data_interp, data, M_data, N_data, x_interp, y_interp, N_interp, isdefault, defaultvalue, 0, num_exterior, kernel_ms);
    (void)nxs_regrid_destroy(r);
    return rc;
} catch (...) { return entry_caught("nxs_interp_mesh_to_mesh_2d"); }

extern "C" int nxs_interp_last_timing(double *ms8) try {
    if (!ms8) return fail(NXS_ERR_INVALID, "NULL argument");
    for (int i = 0; i < 8; ++i) ms8[i] = g_ms[i];
    return NXS_OK;
} catch (...) { return entry_caught("nxs_interp_last_timing"); }

extern "C" int nxs_interp_last_info(int32_t *num_fill_triangles, int32_t *num_hull_edges, int32_t *num_exterior, int32_t *num_in_fill,
                                    int32_t *num_on_hull, int32_t *num_stand_in, const char **completion_refused) try {
    if (num_fill_triangles) *num_fill_triangles = g_info[0];
    if (num_hull_edges) *num_hull_edges = g_info[1];
    if (num_exterior) *num_exterior = g_info[2];
    if (num_in_fill) *num_in_fill = g_info[3];
    if (num_on_hull) *num_on_hull = g_info[4];
    if (num_stand_in) *num_stand_in = g_info[5];
    if (completion_refused) *completion_refused = g_info[6] ? g_completion_note.c_str() : nullptr;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_interp_last_info"); }

// Host only: bamg's convex completion of a mesh (see nxs_hull.inl) -- what tests compare with the real bamg.
// mode 0: the pocket construction, and the general one (constrained Delaunay of the boundary vertices) where that does not apply; 1: the general one; 2: pockets only
extern "C" int nxs_mesh_convex_completion_mode(const int32_t *index, const double *x, const double *y, int32_t nods, int32_t nels,
                                          int32_t *num_fill, int32_t *fill_tri, int32_t cap_fill, int32_t *num_hull, int32_t *hull_edges,
                                          int32_t cap_hull, int32_t mode) try {
    if (!index || !x || !y || nods < 3 || nels < 1 || !num_fill || !num_hull) return fail(NXS_ERR_INVALID, "bad arguments");
    for (int64_t i = 0; i < 3ll * nels; ++i)
        if (index[i] < 1 || index[i] > nods) return fail(NXS_ERR_INVALID, "index[%lld] out of range", (long long)i);
    // SetIntCoor, Mesh.cpp:3441-3468 (as Locator::build)
    double coef = 0., pminx = 0., pminy = 0.;
    std::vector<int> ix, iy;
    if (!nxs_hull::int_plane(x, y, nods, ix, iy, coef, pminx, pminy)) return fail(NXS_ERR_INVALID, "coefIcoor should be positive");
    const nxs_hull::Completion c = nxs_hull::complete_any(index, ix.data(), iy.data(), nods, nels, mode);
    if (!c.ok) return fail(NXS_ERR_INVALID, "no convex completion: %s", c.why.c_str());
    *num_fill = (int)c.fill.size() / 3; *num_hull = (int)c.hull.size();
    if (fill_tri) { if (cap_fill < *num_fill) return fail(NXS_ERR_INVALID, "fill_tri too small"); for (size_t i = 0; i < c.fill.size(); ++i) fill_tri[i] = c.fill[i] + 1; }
    if (hull_edges) {
        if (cap_hull < *num_hull) return fail(NXS_ERR_INVALID, "hull_edges too small");
        for (size_t i = 0; i < c.hull.size(); ++i) { hull_edges[2 * i] = c.hull[i].a + 1; hull_edges[2 * i + 1] = c.hull[i].b + 1; }
    }
    return NXS_OK;
} catch (...) { return entry_caught("nxs_mesh_convex_completion_mode"); }

extern "C" int nxs_mesh_convex_completion(const int32_t *index, const double *x, const double *y, int32_t nods, int32_t nels,
                                          int32_t *num_fill, int32_t *fill_tri, int32_t cap_fill, int32_t *num_hull, int32_t *hull_edges,
                                          int32_t cap_hull) try {
    return nxs_mesh_convex_completion_mode(index, x, y, nods, nels, num_fill, fill_tri, cap_fill, num_hull, hull_edges, cap_hull, 0);
} catch (...) { return entry_caught("nxs_mesh_convex_completion"); }

// ---------------------------------------------------------------------------------------------------------
// Conservative remapping of the element variables at regrid (ConservativeRemappingMeshToMesh, FE.cpp:3108)
// ---------------------------------------------------------------------------------------------------------
#undef NXS_HD
#define NXS_HD __device__
#include "nxs_remap_core.inl"

namespace {

struct RemapDev {
    InterpDev loc;           // old mesh in bamg's integer plane (seed search = InterpFromMeshToMesh2dx with isdefault)
    nxs_remap::OldMesh m;
    int nels_new, nb_var, n_geom;
    const int *tri_new;      // [3*nels_new] 0-based
    const double *xn, *yn;
    const double *prev;      // bamgmesh_new->PreviousNumbering or NULL
};

// one thread per new triangle: seed, identity test, replay of checkTriangle's recursion, weighted sum
__global__ void __launch_bounds__(128) k_remap(RemapDev r, const double *__restrict__ in, double *__restrict__ out, int *failed, int *visits,
                                               int *failed_list, int failed_cap) {
    const int t = blockIdx.x * 128 + threadIdx.x;
    if (t >= r.nels_new) return;
    double cx[3], cy[3];
    int nt[3];
    double gx = 0., gy = 0.;  // barycentre, ConservativeRemapping.cpp:217-231
    for (int i = 0; i < 3; ++i) {
        nt[i] = r.tri_new[3 * t + i];
        cx[i] = r.xn[nt[i]];
        cy[i] = r.yn[nt[i]];
        gx += cx[i];
        gy += cy[i];
    }
    gx /= 3.;
    gy /= 3.;
    double *o = out + (size_t)t * r.nb_var;
    int seed = -1;
    if (!(gx < r.loc.xmin || gx > r.loc.xmax || gy < r.loc.ymin || gy > r.loc.ymax)) {
        long long dd[3], Bx, By;
        seed = locate(r.loc, gx, gy, dd, Bx, By);
    }
    int n = -1;
    int tris[nxs_remap::kMaxVisit];
    double w[nxs_remap::kMaxVisit];
    nxs_remap::Frame stack[nxs_remap::kMaxVisit + 1];
    if (seed >= 0) {
        const bool same = nxs_remap::same_triangle(r.m, seed, nt, r.prev, r.n_geom);
        n = nxs_remap::collect(r.m, cx, cy, seed, same, tris, w, stack);
    }
    if (visits) visits[t] = n;
    if (n < 0) {  // barycentre outside the old mesh (the reference asserts) or capacity exceeded: flagged, never silent
        const int slot = atomicAdd(failed, 1);
        if (failed_list && slot < failed_cap) failed_list[slot] = seed >= 0 ? t : ~t;  // ~t: no seed, nothing a second pass can do
        for (int v = 0; v < r.nb_var; ++v) o[v] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    nxs_remap::apply(in, r.nb_var, cx, cy, tris, w, n, o);
}

// second pass for the new triangles that overlap more than kMaxVisit old ones (a much coarser new mesh): the same
// walk with lists of kMaxVisitBig entries in global memory, one thread per such triangle
__global__ void __launch_bounds__(64) k_remap_big(RemapDev r, const double *__restrict__ in, double *__restrict__ out, const int *__restrict__ list, int nlist,
                                                  int *tris_all, double *w_all, nxs_remap::Frame *stack_all, int *still_failed, int *visits) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= nlist) return;
    const int t = list[i];
    double cx[3], cy[3], gx = 0., gy = 0.;
    int nt[3];
    for (int k = 0; k < 3; ++k) { nt[k] = r.tri_new[3 * t + k]; cx[k] = r.xn[nt[k]]; cy[k] = r.yn[nt[k]]; gx += cx[k]; gy += cy[k]; }
    gx /= 3.; gy /= 3.;
    long long dd[3], Bx, By;
    const int seed = locate(r.loc, gx, gy, dd, Bx, By);
    int *tris = tris_all + (size_t)i * nxs_remap::kMaxVisitBig;
    double *w = w_all + (size_t)i * nxs_remap::kMaxVisitBig;
    nxs_remap::Frame *stack = stack_all + (size_t)i * (nxs_remap::kMaxVisitBig + 1);
    const int n = seed >= 0 ? nxs_remap::collect(r.m, cx, cy, seed, false, tris, w, stack, nxs_remap::kMaxVisitBig) : -1;
    if (visits) visits[t] = n;
    if (n < 0) { atomicAdd(still_failed, 1); return; }
    nxs_remap::apply(in, r.nb_var, cx, cy, tris, w, n, out + (size_t)t * r.nb_var);
}

}  // namespace

// ConservativeRemappingMeshToMesh on the context's (old) mesh.  flags: NXS_REGRID_IN_DEVICE = interp_in is a device pointer ([nels_old][nb_var]),
// NXS_REGRID_OUT_DEVICE = interp_out is ([nels_new][nb_var]) -- the element state of nxs_dyn lives on the device already.
// nec_old / ec_old (may be NULL): bamg's own tables instead of the ones built here.
extern "C" int nxs_regrid_remap_elements(nxs_regrid *rg, double *interp_out, const double *interp_in, int32_t nb_var, const double *nec_old, int32_t nec_width,
                                         const double *ec_old, const int32_t *index_new, const double *x_new, const double *y_new, int32_t nods_new,
                                         int32_t nels_new, const double *previous_numbering, int32_t n_geom_vertices, int32_t flags,
                                         int32_t *num_failed, int32_t *visits, double *kernel_ms) try {
    if (!rg || !interp_out || !interp_in || !index_new || !x_new || !y_new) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nb_var < 1 || nods_new < 3 || nels_new < 1) return fail(NXS_ERR_INVALID, "bad sizes");
    if (nec_old && nec_width < 1) return fail(NXS_ERR_INVALID, "nec_width must be given with the NodalElementConnectivity table");
    if (hipSetDevice(rg->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const int nods_old = rg->nods, nels_old = rg->nels;
    for (int64_t i = 0; i < 3ll * nels_new; ++i)
        if (index_new[i] < 1 || index_new[i] > nods_new) return fail(NXS_ERR_INVALID, "index_new[%lld] out of range", (long long)i);
    if (previous_numbering)
        for (int i = 0; i < nods_new; ++i)
            if (!(previous_numbering[i] >= 0.) || previous_numbering[i] > (double)nods_old) return fail(NXS_ERR_INVALID, "previous_numbering[%d] out of range", i);
    for (double &v : g_ms) v = 0.;
    Tick whole(6);
    if (int rc = regrid_connectivity(rg, nec_old, nec_width, ec_old)) return rc;
    Locator *locp = nullptr;
    if (int rc = regrid_locator(rg, false, &locp)) return rc;
    Locator &loc = *locp;
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    DevBuf<int> dtrin, dfail, dvis;
    DevBuf<double> dxn, dyn, dprev, din, dout;
    if (dtrin.upload(index_new, 3 * (size_t)nels_new) || dxn.upload(x_new, nods_new) ||
        dyn.upload(y_new, nods_new) || (previous_numbering && dprev.upload(previous_numbering, nods_new)) ||
        (!in_dev && din.upload(interp_in, (size_t)nels_old * nb_var)) || (!out_dev && dout.alloc((size_t)nels_new * nb_var)) || dfail.alloc(1) || (visits && dvis.alloc(nels_new)))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(k_add_int, dim3((3 * nels_new + 255) / 256), dim3(256), 0, S(), 3 * nels_new, dtrin.p, -1);
    if (memset_sync(dfail.p, 0, sizeof(int)) != hipSuccess) return fail(NXS_ERR_HIP, "hipMemset failed");
    const double *inp = in_dev ? interp_in : (const double *)din.p;
    double *outp = out_dev ? interp_out : dout.p;

    RemapDev r{};
    r.loc = loc.d;
    r.loc.isdefault = 1;
    r.m = nxs_remap::OldMesh{nels_old, nods_old, rg->dtrio.p, rg->dxo.p, rg->dyo.p, rg->dnec.p, rg->nec_width, rg->dec.p};
    r.nels_new = nels_new; r.nb_var = nb_var; r.n_geom = n_geom_vertices;
    r.tri_new = dtrin.p; r.xn = dxn.p; r.yn = dyn.p; r.prev = previous_numbering ? dprev.p : nullptr;

    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, S());
    const int failed_cap = 1 << 16;
    DevBuf<int> dflist, dstill, dbt;
    DevBuf<double> dbw;
    DevBuf<nxs_remap::Frame> dbs;
    if (dflist.alloc(failed_cap) || dstill.alloc(1) || memset_sync(dstill.p, 0, sizeof(int)) != hipSuccess) return fail(NXS_ERR_HIP, "device allocation failed");
    hipLaunchKernelGGL(k_remap, dim3((nels_new + 127) / 128), dim3(128), 0, S(), r, inp, outp, dfail.p, visits ? dvis.p : nullptr,
                       dflist.p, failed_cap);
    int nf1 = 0;
    if (copy_sync(&nf1, dfail.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    int unrecoverable = 0, nbig = 0;
    if (nf1 > 0) {  // the few that exceeded the fast path's capacity: second pass with large lists in global memory
        std::vector<int> fl(std::min(nf1, failed_cap));
        if (copy_sync(fl.data(), dflist.p, fl.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
        std::vector<int> big;
        for (int v : fl) { if (v >= 0) big.push_back(v); else ++unrecoverable; }
        unrecoverable += nf1 - (int)fl.size();  // more failures than the list holds: left as failures
        std::sort(big.begin(), big.end());
        nbig = (int)big.size();
        const size_t per = (size_t)nxs_remap::kMaxVisitBig;
        if (nbig > 0) {
            if (dflist.p && copy_sync(dflist.p, big.data(), big.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
            if (dbt.alloc(nbig * per) || dbw.alloc(nbig * per) || dbs.alloc(nbig * (per + 1)))
                return fail(NXS_ERR_HIP, "second remapping pass: %d triangles need %zu MB of lists", nbig, nbig * per * 28 >> 20);
            hipLaunchKernelGGL(k_remap_big, dim3((nbig + 63) / 64), dim3(64), 0, S(), r, inp, outp, (const int *)dflist.p, nbig, dbt.p, dbw.p,
                               dbs.p, dstill.p, visits ? dvis.p : nullptr);
        }
    }
    (void)hipEventRecord(e1, S());
    hipError_t err = hipStreamSynchronize(S());
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(NXS_ERR_HIP, "remapping kernel failed: %s", hipGetErrorString(err));
    g_ms[4] += ms;
    if (kernel_ms) *kernel_ms = ms;
    {
        Tick tk(5);
        if (!out_dev && copy_sync(interp_out, dout.p, (size_t)nels_new * nb_var * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
        if (visits && copy_sync(visits, dvis.p, (size_t)nels_new * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    }
    int still = 0;
    (void)copy_sync(&still, dstill.p, sizeof(int), hipMemcpyDeviceToHost);
    if (num_failed) *num_failed = unrecoverable + still;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_regrid_remap_elements"); }

extern "C" int nxs_interp_conservative_remap(double *interp_out, const double *interp_in, int32_t nb_var, const int32_t *index_old,
                                             const double *x_old, const double *y_old, int32_t nods_old, int32_t nels_old,
                                             const double *nec_old, int32_t nec_width, const double *ec_old, const int32_t *index_new,
                                             const double *x_new, const double *y_new, int32_t nods_new, int32_t nels_new,
                                             const double *previous_numbering, int32_t n_geom_vertices, int32_t device,
                                             int32_t *num_failed, int32_t *visits, double *kernel_ms) try {
    if (!interp_out || !interp_in || !index_old || !x_old || !y_old || !index_new || !x_new || !y_new) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nb_var < 1 || nods_old < 3 || nels_old < 1 || nods_new < 3 || nels_new < 1) return fail(NXS_ERR_INVALID, "bad sizes");
    nxs_regrid *r = nullptr;
    if (int rc = regrid_create(index_old, x_old, y_old, nods_old, nels_old, device, &r, false)) return rc;
    const int rc = nxs_regrid_remap_elements(r, interp_out, interp_in, nb_var, nec_old, nec_width, ec_old, index_new, x_new, y_new, nods_new, nels_new,
                                             previous_numbering, n_geom_vertices, 0, num_failed, visits, kernel_ms);
    (void)nxs_regrid_destroy(r);
    return rc;
} catch (...) { return entry_caught("nxs_interp_conservative_remap"); }

// test door: the device-built tables of a context (the bucket grid's offsets and lists; NodalElementConnectivity and ElementConnectivity as ints)
extern "C" int nxs_regrid_debug_tables(nxs_regrid *rg, int32_t which, int32_t *out, int64_t cap, int64_t *count) try {
    if (!rg || !count) return fail(NXS_ERR_INVALID, "NULL argument");
    if (hipSetDevice(rg->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    Locator *loc = nullptr;
    if (which <= 1) { if (int rc = regrid_locator(rg, false, &loc)) return rc; }
    else if (int rc = regrid_connectivity(rg, nullptr, 0, nullptr)) return rc;
    const int *src = nullptr; int64_t n = 0;
    if (which == 0) { src = loc->d.cell_off; n = (int64_t)loc->d.G * loc->d.G + 1; }
    else if (which == 1) { src = loc->d.cell_tri; int tot = 0; (void)copy_sync(&tot, loc->d.cell_off + (size_t)loc->d.G * loc->d.G, sizeof(int), hipMemcpyDeviceToHost); n = tot; }
    else if (which == 2) { src = rg->dnec.p; n = (int64_t)rg->nods * rg->nec_width; }
    else if (which == 3) { src = rg->dec.p; n = 3ll * rg->nels; }
    else return fail(NXS_ERR_INVALID, "which must be 0 .. 3");
    *count = n;
    if (out) {
        if (cap < n) return fail(NXS_ERR_INVALID, "buffer too small (%lld entries)", (long long)n);
        if (n > 0 && copy_sync(out, src, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    }
    return NXS_OK;
} catch (...) { return entry_caught("nxs_regrid_debug_tables"); }

// ---------------------------------------------------------------------------------------------------------
// Conservative remapping between the mesh and a grid of quadrilateral cells, the weights resident as lists (nxs_gridmap_*):
// ConservativeRemappingWeights / MeshToGrid / GridToMesh, contrib/bamg/src/ConservativeRemapping.cpp:15-171
// ---------------------------------------------------------------------------------------------------------
namespace {
#include "nxs_gridmap_kernels.inl"
int g_gridmap_chunk = 0;        // test door (nxs_gridmap_debug_chunk): cells per chunk of the weights build, 0 = as many as the arena allows
int g_gridmap_last_chunks = 0;  // chunks the last nxs_gridmap_create of the process took
int g_gridmap_receive_lists = 1;  // nxs_gridmap_debug_receive_lists: 0 = the receive walks cell / w through t_pos, 1 (the faster on the 2 km mesh: DESIGN 6n) = through copies in transposed order
}  // namespace

struct nxs_gridmap {
    int device = 0, nels = 0, G = 0, rows = 0, longest = 0, failed = 0;
    long long n = 0;                       // entries
    std::vector<double> cornerX, cornerY;  // [4 G], host (nxs_gridmap_export; the device copies are only needed while the map is made)
    DevBuf<int> dgridP, doff, dtris;       // the forward lists: row i is cell gridP[i], entries off[i] .. off[i + 1]
    DevBuf<double> dw, drarea;             // weights; 1 / area(cell) per row
    DevBuf<int> drow_of_cell;              // [G] row of a cell, -1 = land
    DevBuf<int> dt_off, dt_pos, dcell;     // the transposed lists: per triangle the indices of its entries, ascending; the cell of every entry
    DevBuf<int> dcell_t;                   // nxs_gridmap_receive_rows: copies of cell and w in transposed
    DevBuf<double> dw_t;                   // order, made by the first call on the map (12 bytes per entry; not under nxs_gridmap_debug_receive_lists(0))
    DevBuf<double> dstage;                 // ... with host fields: where they are uploaded, [n_var][G]; it only grows
    size_t stage_cap = 0;
};

namespace {

// everything derived from the forward lists (already on the device) and the corners: 1 / area, row_of_cell, the transposed lists
int gridmap_finish(nxs_gridmap *g, const double *dcx, const double *dcy) {
    const int rows = g->rows, nels = g->nels, n = (int)g->n;
    DevBuf<int> cursor;
    if (g->drarea.alloc(rows) || g->drow_of_cell.alloc(g->G) || g->dt_off.alloc((size_t)nels + 1) || g->dt_pos.alloc(n) || g->dcell.alloc(n) || cursor.alloc(nels))
        return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
    if (hipMemsetAsync(g->drow_of_cell.p, 0xff, (size_t)g->G * sizeof(int), S()) != hipSuccess || hipMemsetAsync(g->dt_off.p, 0, ((size_t)nels + 1) * sizeof(int), S()) != hipSuccess ||
        hipMemsetAsync(cursor.p, 0, (size_t)nels * sizeof(int), S()) != hipSuccess)
        return fail(NXS_ERR_HIP, "hipMemset failed");
    if (rows > 0)
        hipLaunchKernelGGL(gridmap::k_gridmap_rows, dim3((rows + 255) / 256), dim3(256), 0, S(), rows, (const int *)g->dgridP.p, dcx, dcy, g->drarea.p, g->drow_of_cell.p);
    if (n > 0) {
        hipLaunchKernelGGL(gridmap::k_gridmap_t_count, dim3((n + 255) / 256), dim3(256), 0, S(), n, (const int *)g->dtris.p, g->dt_off.p);
        if (regrid_tables::exclusive_scan(g->dt_off.p, nels + 1, S()) != hipSuccess) return fail(NXS_ERR_HIP, "scan of the transposed lists failed");
        hipLaunchKernelGGL(gridmap::k_gridmap_t_fill, dim3((n + 255) / 256), dim3(256), 0, S(), n, rows, (const int *)g->dtris.p, (const int *)g->doff.p, (const int *)g->dgridP.p,
                           (const int *)g->dt_off.p, cursor.p, g->dt_pos.p, g->dcell.p);
        hipLaunchKernelGGL(regrid_tables::k_rows_sort, dim3((nels + 255) / 256), dim3(256), 0, S(), nels, (const int *)g->dt_off.p, g->dt_pos.p, 0);
    }
    if (hipStreamSynchronize(S()) != hipSuccess) return fail(NXS_ERR_HIP, "grid map kernels failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// a map out of host lists (nxs_gridmap_import, nxs_gridmap_restrict): checked, uploaded, finished
int gridmap_from_host(int device, int nels, int G, int rows, const int32_t *gridP, const int32_t *off, const int32_t *tris, const double *w, const double *cornerX,
                      const double *cornerY, int failed, nxs_gridmap **out) {
    if (nels < 1 || G < 1 || rows < 0 || rows > G) return fail(NXS_ERR_INVALID, "bad sizes");
    if (off[0] != 0) return fail(NXS_ERR_INVALID, "off[0] must be 0");
    int longest = 0;
    for (int i = 0; i < rows; ++i) {
        if (gridP[i] < 0 || gridP[i] >= G || (i > 0 && gridP[i] <= gridP[i - 1])) return fail(NXS_ERR_INVALID, "gridP[%d] out of range or not ascending", i);
        if (off[i + 1] <= off[i]) return fail(NXS_ERR_INVALID, "row %d is empty or off is not ascending", i);
        longest = std::max(longest, off[i + 1] - off[i]);
    }
    const int n = off[rows];
    for (int e = 0; e < n; ++e)
        if (tris[e] < 0 || tris[e] >= nels) return fail(NXS_ERR_INVALID, "tris[%d] out of range", e);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the grid map has no CPU path");
    if (device < 0 || device >= ndev) return fail(NXS_ERR_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    std::unique_ptr<nxs_gridmap> g(new nxs_gridmap());
    g->device = device; g->nels = nels; g->G = G; g->rows = rows; g->n = n; g->longest = longest; g->failed = failed;
    g->cornerX.assign(cornerX, cornerX + 4 * (size_t)G); g->cornerY.assign(cornerY, cornerY + 4 * (size_t)G);
    DevBuf<double> dcx, dcy;
    if (g->dgridP.upload(gridP, rows) || g->doff.upload(off, (size_t)rows + 1) || g->dtris.upload(tris, n) || g->dw.upload(w, n) || dcx.upload(cornerX, 4 * (size_t)G) ||
        dcy.upload(cornerY, 4 * (size_t)G))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    if (int rc = gridmap_finish(g.get(), dcx.p, dcy.p)) return rc;
    *out = g.release();
    return NXS_OK;
}

struct GridmapHost { std::vector<int32_t> gridP, off, tris; std::vector<double> w; };
int gridmap_download(nxs_gridmap *g, GridmapHost &h) {
    h.gridP.resize(g->rows); h.off.resize((size_t)g->rows + 1); h.tris.resize(g->n); h.w.resize(g->n);
    if (copy_sync(h.off.data(), g->doff.p, h.off.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
        (g->rows > 0 && copy_sync(h.gridP.data(), g->dgridP.p, h.gridP.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) ||
        (g->n > 0 && (copy_sync(h.tris.data(), g->dtris.p, h.tris.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                      copy_sync(h.w.data(), g->dw.p, h.w.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)))
        return fail(NXS_ERR_HIP, "copy back failed");
    return 0;
}

}  // namespace

// ConservativeRemappingWeights on the context's mesh (at rest: the reference builds it on bamgmesh_root after a regrid, where M_UM = 0)
extern "C" int nxs_gridmap_create(nxs_regrid *rg, const double *gridX, const double *gridY, const double *cornerX, const double *cornerY, int32_t G,
                                  nxs_gridmap **out) try {
    if (!out) return fail(NXS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!rg || !gridX || !gridY || !cornerX || !cornerY) return fail(NXS_ERR_INVALID, "NULL argument");
    if (G < 1) return fail(NXS_ERR_INVALID, "the grid has no cell");
    if (hipSetDevice(rg->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    for (double &v : g_ms) v = 0.;
    Tick whole(6);
    if (int rc = regrid_connectivity(rg, nullptr, 0, nullptr)) return rc;
    Locator *locp = nullptr;
    if (int rc = regrid_locator(rg, false, &locp)) return rc;
    std::unique_ptr<nxs_gridmap> g(new nxs_gridmap());
    g->device = rg->device; g->nels = rg->nels; g->G = G;
    g->cornerX.assign(cornerX, cornerX + 4 * (size_t)G); g->cornerY.assign(cornerY, cornerY + 4 * (size_t)G);
    DevBuf<double> dgx, dgy, dcx, dcy;
    DevBuf<int> dseed, dcells, dcount, dfailed;
    if (dgx.upload(gridX, G) || dgy.upload(gridY, G) || dcx.upload(cornerX, 4 * (size_t)G) || dcy.upload(cornerY, 4 * (size_t)G) || dseed.alloc(G) || dfailed.alloc(1))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    InterpDev loc = locp->d;
    loc.isdefault = 1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    struct Events { hipEvent_t &a, &b; ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } events{e0, e1};
    (void)hipEventRecord(e0, S());
    hipLaunchKernelGGL(gridmap::k_gridmap_seed, dim3((G + 255) / 256), dim3(256), 0, S(), loc, (int)G, (const double *)dgx.p, (const double *)dgy.p, dseed.p);
    std::vector<int> seed(G), wet;
    if (copy_sync(seed.data(), dseed.p, (size_t)G * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "seed kernel failed: %s", hipGetErrorString(hipGetLastError()));
    for (int c = 0; c < G; ++c) if (seed[c] >= 0) wet.push_back(c);
    const int nwet = (int)wet.size();
    // the walk, in chunks of cells whose arena of kMaxVisitBig-entry lists stays under 2 GiB; every chunk is compacted into a piece of its own
    const size_t K = (size_t)nxs_remap::kMaxVisitBig, per_cell = K * (sizeof(int) + sizeof(double)) + (K + 1) * sizeof(nxs_remap::Frame);
    int chunk = (int)std::min<size_t>((size_t)std::max(nwet, 1), ((size_t)2 << 30) / per_cell - 1);
    if (g_gridmap_chunk > 0) chunk = std::min(chunk, g_gridmap_chunk);
    struct Piece { DevBuf<int> t; DevBuf<double> w; int n = 0; };
    std::vector<std::unique_ptr<Piece>> pieces;
    std::vector<int> count(nwet);
    DevBuf<int> arena_t;
    DevBuf<double> arena_w;
    DevBuf<nxs_remap::Frame> arena_s;
    const nxs_remap::OldMesh m{rg->nels, rg->nods, rg->dtrio.p, rg->dxo.p, rg->dyo.p, rg->dnec.p, rg->nec_width, rg->dec.p};
    if (memset_sync(dfailed.p, 0, sizeof(int)) != hipSuccess) return fail(NXS_ERR_HIP, "hipMemset failed");
    long long total = 0;
    int nchunks = 0;
    if (nwet > 0) {
        if (dcells.upload(wet.data(), nwet) || dcount.alloc((size_t)chunk + 1) || arena_t.alloc(chunk * K) || arena_w.alloc(chunk * K) || arena_s.alloc(chunk * (K + 1)))
            return fail(NXS_ERR_HIP, "weights build: %d cells per chunk need %zu MB of lists", chunk, chunk * per_cell >> 20);
        for (int c0 = 0; c0 < nwet; c0 += chunk, ++nchunks) {
            const int nc = std::min(chunk, nwet - c0);
            if (hipMemsetAsync(dcount.p, 0, ((size_t)nc + 1) * sizeof(int), S()) != hipSuccess) return fail(NXS_ERR_HIP, "hipMemset failed");
            hipLaunchKernelGGL(gridmap::k_gridmap_walk, dim3((nc + 63) / 64), dim3(64), 0, S(), m, nc, (const int *)dcells.p + c0, (const int *)dseed.p, (const double *)dcx.p,
                               (const double *)dcy.p, arena_t.p, arena_w.p, arena_s.p, dcount.p, dfailed.p);
            if (copy_sync(count.data() + c0, dcount.p, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(NXS_ERR_HIP, "weights kernel failed: %s", hipGetErrorString(hipGetLastError()));
            if (regrid_tables::exclusive_scan(dcount.p, nc + 1, S()) != hipSuccess) return fail(NXS_ERR_HIP, "scan of the row lengths failed");
            std::unique_ptr<Piece> p(new Piece());
            for (int i = 0; i < nc; ++i) p->n += count[c0 + i];
            if (p->n > 0) {
                if (p->t.alloc(p->n) || p->w.alloc(p->n)) return fail(NXS_ERR_HIP, "device allocation failed");
                hipLaunchKernelGGL(gridmap::k_gridmap_compact, dim3((nc + 3) / 4), dim3(256), 0, S(), nc, (const int *)dcount.p, (const int *)arena_t.p, (const double *)arena_w.p,
                                   p->t.p, p->w.p);
            }
            total += p->n;
            pieces.push_back(std::move(p));
        }
    }
    g_gridmap_last_chunks = nchunks;
    if (total > 0x7fffffffll) return fail(NXS_ERR_INVALID, "the lists have %lld entries (int offsets)", total);
    if (copy_sync(&g->failed, dfailed.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "weights kernel failed: %s", hipGetErrorString(hipGetLastError()));
    // the rows: wet cells that were not failed, in cell order; the scan across the chunks
    std::vector<int> gridP, off(1, 0);
    for (int i = 0; i < nwet; ++i)
        if (count[i] > 0) { gridP.push_back(wet[i]); off.push_back(off.back() + count[i]); g->longest = std::max(g->longest, count[i]); }
    g->rows = (int)gridP.size(); g->n = total;
    if (g->dtris.alloc(total) || g->dw.alloc(total) || g->dgridP.upload(gridP.data(), gridP.size()) || g->doff.upload(off.data(), off.size()))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    size_t base = 0;
    for (const auto &p : pieces) {
        if (p->n > 0 && (hipMemcpyAsync(g->dtris.p + base, p->t.p, (size_t)p->n * sizeof(int), hipMemcpyDeviceToDevice, S()) != hipSuccess ||
                         hipMemcpyAsync(g->dw.p + base, p->w.p, (size_t)p->n * sizeof(double), hipMemcpyDeviceToDevice, S()) != hipSuccess))
            return fail(NXS_ERR_HIP, "device copy failed");
        base += p->n;
    }
    if (int rc = gridmap_finish(g.get(), dcx.p, dcy.p)) return rc;
    (void)hipEventRecord(e1, S());
    if (hipStreamSynchronize(S()) != hipSuccess) return fail(NXS_ERR_HIP, "grid map kernels failed: %s", hipGetErrorString(hipGetLastError()));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    g_ms[4] += ms;
    *out = g.release();
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_create"); }

extern "C" int nxs_gridmap_destroy(nxs_gridmap *g) try {
    if (!g) return NXS_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_destroy"); }

extern "C" int nxs_gridmap_info(const nxs_gridmap *g, int32_t *wet_cells, int64_t *entries, int32_t *longest_row, int32_t *failed_cells, int32_t *nels,
                                int32_t *grid_size) try {
    if (!g) return fail(NXS_ERR_INVALID, "NULL argument");
    if (wet_cells) *wet_cells = g->rows;
    if (entries) *entries = g->n;
    if (longest_row) *longest_row = g->longest;
    if (failed_cells) *failed_cells = g->failed;
    if (nels) *nels = g->nels;
    if (grid_size) *grid_size = g->G;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_info"); }

// ConservativeRemappingMeshToGrid (:103-135).  flags: NXS_REGRID_IN_DEVICE = `in` is a device pointer ([nels][nb_var]), NXS_REGRID_OUT_DEVICE = `out` is ([G][nb_var])
extern "C" int nxs_gridmap_mesh_to_grid(nxs_gridmap *g, double *out, const double *in, int32_t nb_var, double miss_val, int32_t flags) try {
    if (!g || !out || !in) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nb_var < 1) return fail(NXS_ERR_INVALID, "nb_var must be positive");
    if (hipSetDevice(g->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    const long long total = (long long)g->G * nb_var;
    DevBuf<double> din, dout;
    if ((!in_dev && din.upload(in, (size_t)g->nels * nb_var)) || (!out_dev && dout.alloc((size_t)total)))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    double *outp = out_dev ? out : dout.p;
    hipLaunchKernelGGL(gridmap::k_gridmap_to_grid, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(), total, (int)nb_var, (const int *)g->drow_of_cell.p, (const int *)g->doff.p,
                       (const int *)g->dtris.p, (const double *)g->dw.p, (const double *)g->drarea.p, in_dev ? in : (const double *)din.p, miss_val, outp);
    if (hipStreamSynchronize(S()) != hipSuccess) return fail(NXS_ERR_HIP, "mesh-to-grid kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (!out_dev && copy_sync(out, dout.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_mesh_to_grid"); }

// ConservativeRemappingGridToMesh (:138-171) as a gather.  flags as above: `in` [G][nb_var], `out` [nels][nb_var]
extern "C" int nxs_gridmap_grid_to_mesh(nxs_gridmap *g, double *out, const double *in, int32_t nb_var, int32_t flags) try {
    if (!g || !out || !in) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nb_var < 1) return fail(NXS_ERR_INVALID, "nb_var must be positive");
    if (hipSetDevice(g->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    const long long total = (long long)g->nels * nb_var;
    DevBuf<double> din, dout;
    if ((!in_dev && din.upload(in, (size_t)g->G * nb_var)) || (!out_dev && dout.alloc((size_t)total)))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    double *outp = out_dev ? out : dout.p;
    hipLaunchKernelGGL(gridmap::k_gridmap_to_mesh, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(), total, (int)nb_var, (const int *)g->dt_off.p, (const int *)g->dt_pos.p,
                       (const int *)g->dcell.p, (const double *)g->dw.p, in_dev ? in : (const double *)din.p, outp);
    if (hipStreamSynchronize(S()) != hipSuccess) return fail(NXS_ERR_HIP, "grid-to-mesh kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (!out_dev && copy_sync(out, dout.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_grid_to_mesh"); }

// The coupler's receive: receiveCouplingData's transform, ConservativeRemappingGridToMesh and ExternalData::get's factor / bias in one launch on `stream`
// (dataset.cpp:2828-3031, ConservativeRemapping.cpp:138-171, externaldata.cpp:434-438).  fields [n_var] of [G], out_rows [n_var] of [nels]
extern "C" int nxs_gridmap_receive_rows(nxs_gridmap *g, int32_t n_var, const double *const *fields, const double *a, const double *b, const double *factor,
                                        const double *bias, double *const *out_rows, int32_t flags, void *stream) try {
    if (!g || !fields || !a || !b || !factor || !bias || !out_rows) return fail(NXS_ERR_INVALID, "receive_rows: NULL argument");
    if (n_var < 1 || n_var > gridmap::kMaxReceive) return fail(NXS_ERR_INVALID, "receive_rows: n_var = %d (1 .. %d)", n_var, gridmap::kMaxReceive);
    for (int v = 0; v < n_var; ++v)
        if (!fields[v] || !out_rows[v]) return fail(NXS_ERR_INVALID, "receive_rows: %s %d is NULL", fields[v] ? "output row" : "field", v);
    if (hipSetDevice(g->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    const hipStream_t st = stream ? (hipStream_t)stream : S();
    const size_t G = (size_t)g->G, nels = (size_t)g->nels;
    const bool perm = g_gridmap_receive_lists == 1 && g->n > 0;
    if (perm && !g->dcell_t.p) {
        if (g->dcell_t.alloc(g->n) || g->dw_t.alloc(g->n)) return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        hipLaunchKernelGGL(gridmap::k_gridmap_permute, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, st, (int)g->n, (const int *)g->dt_pos.p, (const int *)g->dcell.p,
                           (const double *)g->dw.p, g->dcell_t.p, g->dw_t.p);
        if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "permuting the lists failed: %s", hipGetErrorString(hipGetLastError()));   // (once: a later call may come on another stream)
    }
    gridmap::ReceiveArgs r{};
    DevBuf<double> dout;
    if (!in_dev) {   // the fields go up on the same stream; the host arrays are the caller's again on return
        if (g->stage_cap < (size_t)n_var * G) {
            if (g->dstage.alloc((size_t)n_var * G)) { g->stage_cap = 0; return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError())); }
            g->stage_cap = (size_t)n_var * G;
        }
        for (int v = 0; v < n_var; ++v)
            if (hipMemcpyAsync(g->dstage.p + (size_t)v * G, fields[v], G * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
    if (!out_dev && dout.alloc((size_t)n_var * nels)) return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
    for (int v = 0; v < n_var; ++v) {
        r.field[v] = in_dev ? fields[v] : g->dstage.p + (size_t)v * G;
        r.out[v] = out_dev ? out_rows[v] : dout.p + (size_t)v * nels;
        r.co[v] = nxs_remap::ReceiveCoef{a[v], b[v], factor[v], bias[v]};
    }
    const dim3 grid((unsigned)((nels + 255) / 256)), block(256);
    const int *t_off = g->dt_off.p, *t_pos = g->dt_pos.p, *cell = perm ? g->dcell_t.p : g->dcell.p;
    const double *w = perm ? g->dw_t.p : g->dw.p;
#define NXS_RECEIVE(NV)                                                                                                             \
    case NV:                                                                                                                        \
        if (perm) hipLaunchKernelGGL((gridmap::k_gridmap_receive<NV, true>), grid, block, 0, st, (int)nels, t_off, t_pos, cell, w, r);  \
        else hipLaunchKernelGGL((gridmap::k_gridmap_receive<NV, false>), grid, block, 0, st, (int)nels, t_off, t_pos, cell, w, r);      \
        break;
    switch (n_var) { NXS_RECEIVE(1) NXS_RECEIVE(2) NXS_RECEIVE(3) NXS_RECEIVE(4) NXS_RECEIVE(5) }
#undef NXS_RECEIVE
    if (hipGetLastError() != hipSuccess) return fail(NXS_ERR_HIP, "receive kernel launch failed");
    if (stream && out_dev) return NXS_OK;   // asynchronous on the caller's stream
    if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "receive kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (!out_dev)
        for (int v = 0; v < n_var; ++v)
            if (copy_sync(out_rows[v], dout.p + (size_t)v * nels, nels * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_receive_rows"); }

// The coupler's put: GridOutput::updateGridMean's conservative elemental leg (gridoutput.cpp:473, 545; ConservativeRemapping.cpp:103-135), ADDED to the [n_var][G]
// rows of data_grid.  in [nels][n_var].  Column tiles of gridmap::kSendTile; the builds for at most 4, 8 and 12 variables
extern "C" int nxs_gridmap_send_rows(nxs_gridmap *g, int32_t n_var, const double *in, double *data_grid, int32_t flags, void *stream) try {
    if (!g || !in || !data_grid) return fail(NXS_ERR_INVALID, "send_rows: NULL argument");
    if (n_var < 1) return fail(NXS_ERR_INVALID, "send_rows: n_var = %d must be positive", n_var);
    if (hipSetDevice(g->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    const hipStream_t st = stream ? (hipStream_t)stream : S();
    const size_t G = (size_t)g->G, nels = (size_t)g->nels;
    DevBuf<double> din, dout;
    if ((!in_dev && din.alloc(nels * n_var)) || (!out_dev && dout.alloc(G * n_var))) return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
    if ((!in_dev && hipMemcpyAsync(din.p, in, nels * n_var * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) ||
        (!out_dev && hipMemcpyAsync(dout.p, data_grid, G * n_var * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess))
        return fail(NXS_ERR_HIP, "upload failed");
    const double *inp = in_dev ? in : (const double *)din.p;
    double *outp = out_dev ? data_grid : dout.p;
    const dim3 grid((unsigned)((G + 255) / 256)), block(256);
    for (int col0 = 0; col0 < n_var; col0 += gridmap::kSendTile) {
        const int nv = std::min<int>(gridmap::kSendTile, n_var - col0);
#define NXS_SEND(NV)                                                                                                                                                   \
        hipLaunchKernelGGL((gridmap::k_gridmap_send<NV>), grid, block, 0, st, (int)G, (int)n_var, col0, nv, (const int *)g->drow_of_cell.p, (const int *)g->doff.p, \
                           (const int *)g->dtris.p, (const double *)g->dw.p, (const double *)g->drarea.p, inp, outp)
        if (nv <= 4) NXS_SEND(4); else if (nv <= 8) NXS_SEND(8); else NXS_SEND(12);
#undef NXS_SEND
    }
    if (hipGetLastError() != hipSuccess) return fail(NXS_ERR_HIP, "send kernel launch failed");
    if (stream && in_dev && out_dev) return NXS_OK;   // asynchronous on the caller's stream
    if (!out_dev && hipMemcpyAsync(data_grid, dout.p, G * n_var * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "send kernel failed: %s", hipGetErrorString(hipGetLastError()));
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_send_rows"); }

// test door: how nxs_gridmap_receive_rows reads cell / w -- 0 through t_pos, 1 through copies in transposed order; *previous (may be NULL) = the mode before
extern "C" int nxs_gridmap_debug_receive_lists(int32_t mode, int32_t *previous) try {
    if (mode != 0 && mode != 1) return fail(NXS_ERR_INVALID, "mode must be 0 or 1");
    if (previous) *previous = g_gridmap_receive_lists;
    g_gridmap_receive_lists = mode;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_debug_receive_lists"); }

// the host form of the lists for the caller's broadcast; sizes from nxs_gridmap_info; any pointer may be NULL
extern "C" int nxs_gridmap_export(nxs_gridmap *g, int32_t *gridP, int32_t *off, int32_t *tris, double *w, double *cornerX, double *cornerY) try {
    if (!g) return fail(NXS_ERR_INVALID, "NULL argument");
    if (hipSetDevice(g->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    GridmapHost h;
    if (int rc = gridmap_download(g, h)) return rc;
    if (gridP) std::copy(h.gridP.begin(), h.gridP.end(), gridP);
    if (off) std::copy(h.off.begin(), h.off.end(), off);
    if (tris) std::copy(h.tris.begin(), h.tris.end(), tris);
    if (w) std::copy(h.w.begin(), h.w.end(), w);
    if (cornerX) std::copy(g->cornerX.begin(), g->cornerX.end(), cornerX);
    if (cornerY) std::copy(g->cornerY.begin(), g->cornerY.end(), cornerY);
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_export"); }

extern "C" int nxs_gridmap_import(int32_t device, int32_t nels, int32_t G, int32_t rows, const int32_t *gridP, const int32_t *off, const int32_t *tris, const double *w,
                                  const double *cornerX, const double *cornerY, nxs_gridmap **out) try {
    if (!out) return fail(NXS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!off || !cornerX || !cornerY || (rows > 0 && (!gridP || !tris || !w))) return fail(NXS_ERR_INVALID, "NULL argument");
    return gridmap_from_host(device, nels, G, rows, gridP, off, tris, w, cornerX, cornerY, 0, out);
} catch (...) { return entry_caught("nxs_gridmap_import"); }

// gridoutput.cpp:706-735: the entries of local triangles, renumbered; rows left empty dropped
extern "C" int nxs_gridmap_restrict(nxs_gridmap *g, const int32_t *local_of_root, int32_t nels_local, nxs_gridmap **out) try {
    if (!out) return fail(NXS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!g || !local_of_root) return fail(NXS_ERR_INVALID, "NULL argument");
    if (nels_local < 1) return fail(NXS_ERR_INVALID, "nels_local must be positive");
    for (int t = 0; t < g->nels; ++t)
        if (local_of_root[t] >= nels_local) return fail(NXS_ERR_INVALID, "local_of_root[%d] = %d is not below nels_local", t, local_of_root[t]);
    if (hipSetDevice(g->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    GridmapHost h, r;
    if (int rc = gridmap_download(g, h)) return rc;
    r.off.push_back(0);
    for (int i = 0; i < g->rows; ++i) {
        for (int k = h.off[i]; k < h.off[i + 1]; ++k) {
            const int loc = local_of_root[h.tris[k]];
            if (loc >= 0) { r.tris.push_back(loc); r.w.push_back(h.w[k]); }
        }
        if ((int)r.tris.size() > r.off.back()) { r.gridP.push_back(h.gridP[i]); r.off.push_back((int32_t)r.tris.size()); }
    }
    return gridmap_from_host(g->device, nels_local, g->G, (int)r.gridP.size(), r.gridP.data(), r.off.data(), r.tris.data(), r.w.data(), g->cornerX.data(), g->cornerY.data(),
                             g->failed, out);
} catch (...) { return entry_caught("nxs_gridmap_restrict"); }

// test door: the weights build in chunks of `cells` cells (0 = as many as the 2 GiB arena allows); *last_chunks = the chunks the last build took
extern "C" int nxs_gridmap_debug_chunk(int32_t cells, int32_t *last_chunks) try {
    if (cells < 0) return fail(NXS_ERR_INVALID, "cells must not be negative");
    g_gridmap_chunk = cells;
    if (last_chunks) *last_chunks = g_gridmap_last_chunks;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_gridmap_debug_chunk"); }

// ---------------------------------------------------------------------------------------------------------
// The coupler's receive of nodal fields: InterpFromMeshToMesh2dx_weights once per mesh, _apply per coupling step (nxs_nodemap_*, include/nxs_interp.h)
// ---------------------------------------------------------------------------------------------------------
namespace {
#include "nxs_nodemap_kernels.inl"
#include "nxs_nodemap_load_kernels.inl"
}  // namespace

struct nxs_nodemap {
    int device = 0, N = 0, nods = 0, beyond_hull = 0;
    DevBuf<int> v0, v1, v2;            // [N] the 0-based source vertices of every target
    DevBuf<double> a0, a1, a2;         // [N] their area coordinates
    // the source side (nxs_nodemap_set_source)
    bool have_source = false;
    int G = 0, R = 0, rotate = 0, east_west = 0;
    bool identity = true;
    double c = 1., s = 0.;
    nxs_mapx_polar map{};
    DevBuf<int> dreduced;
    DevBuf<double> dcs, dsn, dlat, dlon;
    DevBuf<double> dstage;             // [NXS_NODEMAP_MAX_RECEIVE][R] loaded_data, made by set_source
    DevBuf<double> dfields;            // with host fields: where they are uploaded, [n_var][G]; it only grows
    size_t fields_cap = 0;
    int last_n_var = 0;
    DevBuf<double> dload;              // [n_step*n_var][R] loaded_data of nxs_nodemap_load_rows, made by the first load (a map that never loads has none); it only grows
    size_t load_cap = 0;
    int last_load_cols = 0;
};

namespace {

int nodemap_alloc(nxs_nodemap *m) {
    const size_t N = (size_t)m->N;
    if (m->v0.alloc(N) || m->v1.alloc(N) || m->v2.alloc(N) || m->a0.alloc(N) || m->a1.alloc(N) || m->a2.alloc(N))
        return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

}  // namespace

extern "C" int nxs_nodemap_create(nxs_regrid *src, const double *x, const double *y, int32_t N, int32_t flags, nxs_nodemap **out) try {
    if (!out) return fail(NXS_ERR_INVALID, "nodemap_create: out is NULL");
    *out = nullptr;
    if (!src || !x || !y) return fail(NXS_ERR_INVALID, "nodemap_create: NULL argument");
    if (N < 1) return fail(NXS_ERR_INVALID, "nodemap_create: N = %d must be positive", N);
    if (flags != 0) return fail(NXS_ERR_INVALID, "nodemap_create: flags = %d (0 expected)", flags);
    if (hipSetDevice(src->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    Locator *locp = nullptr;
    if (int rc = regrid_locator(src, true, &locp)) return rc;
    if (!locp->comp.ok || locp->d.nhull < 1)
        return fail(NXS_ERR_INVALID, "nodemap_create: the source triangulation has no convex completion (%s): a map never holds stand-in weights",
                    locp->comp.why.empty() ? "no hull edge" : locp->comp.why.c_str());
    std::unique_ptr<nxs_nodemap> m(new nxs_nodemap());
    m->device = src->device; m->N = N; m->nods = src->nods;
    if (int rc = nodemap_alloc(m.get())) return rc;
    DevBuf<double> dx, dy;
    DevBuf<int> dcounts;
    const int counts0[4] = {0, 0x7fffffff, 0, 0};
    if (dx.upload(x, N) || dy.upload(y, N) || dcounts.upload(counts0, 4)) return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    InterpDev d = locp->d;
    d.N_data = 0; d.N_interp = N; d.nodal = 1; d.isdefault = 0; d.defaultvalue = 0.;
    hipLaunchKernelGGL(nodemap::k_nodemap_weights, dim3((N + 255) / 256), dim3(256), 0, S(), d, (const double *)dx.p, (const double *)dy.p,
                       nodemap::Weights{m->v0.p, m->v1.p, m->v2.p, m->a0.p, m->a1.p, m->a2.p}, dcounts.p);
    int counts[4] = {0, 0, 0, 0};
    if (copy_sync(counts, dcounts.p, sizeof counts, hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "weights kernel failed: %s", hipGetErrorString(hipGetLastError()));
    if (counts[0] > 0)   // _weights.cpp:72-73
        return fail(NXS_ERR_INVALID, "nodemap_create: %d target%s outside of the source mesh but inside its convex hull (the first: target %d at %.17g, %.17g): "
                    "InterpFromMeshToMesh2dx_weights throws there", counts[0], counts[0] == 1 ? " is" : "s are", counts[1], x[counts[1]], y[counts[1]]);
    if (counts[3] > 0) return fail(NXS_ERR_INVALID, "nodemap_create: %d targets beyond the hull that no hull edge faces", counts[3]);
    m->beyond_hull = counts[2];
    *out = m.release();
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_create"); }

extern "C" int nxs_nodemap_destroy(nxs_nodemap *m) try {
    if (!m) return NXS_OK;
    (void)hipSetDevice(m->device);
    delete m;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_destroy"); }

extern "C" int nxs_nodemap_info(const nxs_nodemap *m, int32_t *N, int32_t *nods_src, int32_t *beyond_hull) try {
    if (!m) return fail(NXS_ERR_INVALID, "nodemap_info: NULL argument");
    if (N) *N = m->N;
    if (nods_src) *nods_src = m->nods;
    if (beyond_hull) *beyond_hull = m->beyond_hull;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_info"); }

extern "C" int nxs_nodemap_device(const nxs_nodemap *m, int32_t *device) try {
    if (!m || !device) return fail(NXS_ERR_INVALID, "nodemap_device: NULL argument");
    *device = m->device;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_device"); }

extern "C" int nxs_nodemap_export(nxs_nodemap *m, int32_t *v0, int32_t *v1, int32_t *v2, double *a0, double *a1, double *a2) try {
    if (!m) return fail(NXS_ERR_INVALID, "nodemap_export: NULL argument");
    if (hipSetDevice(m->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const size_t N = (size_t)m->N;
    int32_t *vi[3] = {v0, v1, v2};
    const int *vd[3] = {m->v0.p, m->v1.p, m->v2.p};
    double *ai[3] = {a0, a1, a2};
    const double *ad[3] = {m->a0.p, m->a1.p, m->a2.p};
    for (int k = 0; k < 3; ++k) {
        if (vi[k] && copy_sync(vi[k], vd[k], N * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
        if (ai[k] && copy_sync(ai[k], ad[k], N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    }
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_export"); }

extern "C" int nxs_nodemap_import(int32_t device, int32_t N, int32_t nods_src, const int32_t *v0, const int32_t *v1, const int32_t *v2, const double *a0,
                                  const double *a1, const double *a2, nxs_nodemap **out) try {
    if (!out) return fail(NXS_ERR_INVALID, "nodemap_import: out is NULL");
    *out = nullptr;
    if (!v0 || !v1 || !v2 || !a0 || !a1 || !a2) return fail(NXS_ERR_INVALID, "nodemap_import: NULL argument");
    if (N < 1 || nods_src < 1) return fail(NXS_ERR_INVALID, "nodemap_import: N = %d, nods_src = %d must be positive", N, nods_src);
    const int32_t *vi[3] = {v0, v1, v2};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < N; ++i)
            if (vi[k][i] < 0 || vi[k][i] >= nods_src) return fail(NXS_ERR_INVALID, "nodemap_import: v%d[%d] = %d is not a source node (0 .. %d)", k, i, vi[k][i], nods_src - 1);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the node map has no CPU path");
    if (device < 0 || device >= ndev) return fail(NXS_ERR_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    std::unique_ptr<nxs_nodemap> m(new nxs_nodemap());
    m->device = device; m->N = N; m->nods = nods_src;
    if (m->v0.upload(v0, N) || m->v1.upload(v1, N) || m->v2.upload(v2, N) || m->a0.upload(a0, N) || m->a1.upload(a1, N) || m->a2.upload(a2, N))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    m->beyond_hull = -1;   // (not known to an imported map: weights inside a triangle and on a hull edge look alike)
    *out = m.release();
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_import"); }

extern "C" int nxs_nodemap_set_source(nxs_nodemap *m, const nxs_nodemap_source *s) try {
    if (!m || !s) return fail(NXS_ERR_INVALID, "nodemap_set_source: NULL argument");
    if (s->R != m->nods) return fail(NXS_ERR_INVALID, "nodemap_set_source: R = %d, the map's source has %d nodes", s->R, m->nods);
    if (s->G < s->R) return fail(NXS_ERR_INVALID, "nodemap_set_source: G = %d is smaller than R = %d", s->G, s->R);
    if (!s->reduced && s->G != s->R) return fail(NXS_ERR_INVALID, "nodemap_set_source: reduced is NULL (the identity) but G = %d and R = %d differ", s->G, s->R);
    const size_t R = (size_t)s->R;
    if (s->reduced)
        for (size_t i = 0; i < R; ++i)
            if (s->reduced[i] < 0 || s->reduced[i] >= s->G) return fail(NXS_ERR_INVALID, "nodemap_set_source: reduced[%d] = %d is not in 0 .. %d", (int)i, s->reduced[i], s->G - 1);
    if (s->rotation_mode != NXS_NODEMAP_ROTATE_NONE && s->rotation_mode != NXS_NODEMAP_ROTATE_UNIFORM && s->rotation_mode != NXS_NODEMAP_ROTATE_GRID_THETA)
        return fail(NXS_ERR_INVALID, "nodemap_set_source: rotation_mode = %d is not an NXS_NODEMAP_ROTATE_* mode", s->rotation_mode);
    if (s->rotation_mode == NXS_NODEMAP_ROTATE_UNIFORM && (!std::isfinite(s->cos_m_diff_angle) || !std::isfinite(s->sin_m_diff_angle)))
        return fail(NXS_ERR_INVALID, "nodemap_set_source: cos_m_diff_angle / sin_m_diff_angle is not finite");
    if (s->rotation_mode == NXS_NODEMAP_ROTATE_GRID_THETA && !s->theta) return fail(NXS_ERR_INVALID, "nodemap_set_source: NXS_NODEMAP_ROTATE_GRID_THETA needs theta");
    if (s->east_west_oriented) {
        if (!s->lat || !s->lon || !s->map) return fail(NXS_ERR_INVALID, "nodemap_set_source: east_west_oriented needs lat, lon and map");
        if (s->delta_t != 1.) return fail(NXS_ERR_INVALID, "nodemap_set_source: delta_t = %g (the reference's constant is 1.)", s->delta_t);
    }
    std::vector<double> cs, sn;
    if (s->rotation_mode == NXS_NODEMAP_ROTATE_GRID_THETA) {   // externaldata.cpp:1272-1273, on the host
        cs.resize(R); sn.resize(R);
        for (size_t i = 0; i < R; ++i) {
            nxs_cos_sin_of_difference(s->rotation, s->theta[i], &cs[i], &sn[i]);
            if (!std::isfinite(cs[i]) || !std::isfinite(sn[i])) return fail(NXS_ERR_INVALID, "nodemap_set_source: the angle of source point %d is not finite", (int)i);
        }
    }
    if (hipSetDevice(m->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail(NXS_ERR_HIP, "hipDeviceSynchronize failed");   // (a receive on any stream may still read the previous source)
    m->have_source = false;
    if ((s->reduced && m->dreduced.upload(s->reduced, R)) || (!cs.empty() && (m->dcs.upload(cs.data(), R) || m->dsn.upload(sn.data(), R))) ||
        (s->east_west_oriented && (m->dlat.upload(s->lat, R) || m->dlon.upload(s->lon, R))) || m->dstage.alloc((size_t)NXS_NODEMAP_MAX_RECEIVE * R))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    m->G = s->G; m->R = s->R; m->identity = s->reduced == nullptr;
    m->rotate = s->rotation_mode; m->east_west = s->east_west_oriented != 0;
    m->c = s->cos_m_diff_angle; m->s = s->sin_m_diff_angle;
    if (s->east_west_oriented) m->map = *s->map;
    m->last_n_var = 0; m->last_load_cols = 0;
    m->have_source = true;
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_set_source"); }

extern "C" int nxs_nodemap_receive_rows(nxs_nodemap *m, int32_t n_var, const double *const *fields, const double *a, const double *b, const int32_t *pairs,
                                        const double *factor, const double *bias, double *const *out_rows, int32_t flags, void *stream) try {
    if (!m || !fields || !a || !b || !factor || !bias || !out_rows) return fail(NXS_ERR_INVALID, "nodemap_receive_rows: NULL argument");
    if (n_var < 1 || n_var > nodemap::kMaxVar) return fail(NXS_ERR_INVALID, "nodemap_receive_rows: n_var = %d (1 .. %d)", n_var, nodemap::kMaxVar);
    for (int v = 0; v < n_var; ++v)
        if (!fields[v] || !out_rows[v]) return fail(NXS_ERR_INVALID, "nodemap_receive_rows: %s %d is NULL", fields[v] ? "output row" : "field", v);
    if (!m->have_source) return fail(NXS_ERR_STATE, "nodemap_receive_rows: before nxs_nodemap_set_source");
    nodemap::SourceArgs sa{};
    if (pairs) {
        int used[nodemap::kMaxVar] = {0, 0, 0, 0};
        for (int v = 0; v < n_var; ++v) {
            const int w = pairs[v];
            if (w < 0) continue;
            if (w >= n_var || w == v) return fail(NXS_ERR_INVALID, "nodemap_receive_rows: pairs[%d] = %d is not another variable (0 .. %d)", v, w, n_var - 1);
            if (used[v] || used[w]) return fail(NXS_ERR_INVALID, "nodemap_receive_rows: variable %d is named by two pairs", used[v] ? v : w);
            used[v] = used[w] = 1;
            sa.j0[sa.npairs] = v; sa.j1[sa.npairs] = w; ++sa.npairs;   // (four variables hold at most two pairs)
        }
    }
    if (hipSetDevice(m->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    const hipStream_t st = stream ? (hipStream_t)stream : S();
    const size_t G = (size_t)m->G, N = (size_t)m->N;
    if (!in_dev) {   // the fields go up on the same stream; the host arrays are the caller's again on return
        if (m->fields_cap < (size_t)n_var * G) {
            if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "hipStreamSynchronize failed");   // (an earlier receive may still read the buffer)
            if (m->dfields.alloc((size_t)n_var * G)) { m->fields_cap = 0; return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError())); }
            m->fields_cap = (size_t)n_var * G;
        }
        for (int v = 0; v < n_var; ++v)
            if (hipMemcpyAsync(m->dfields.p + (size_t)v * G, fields[v], G * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
    DevBuf<double> dout;
    if (!out_dev && dout.alloc((size_t)n_var * N)) return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
    nodemap::GatherArgs ga{};
    for (int v = 0; v < n_var; ++v) {
        sa.field[v] = in_dev ? fields[v] : m->dfields.p + (size_t)v * G;
        sa.a[v] = a[v]; sa.b[v] = b[v];
        ga.out[v] = out_dev ? out_rows[v] : dout.p + (size_t)v * N;
        ga.factor[v] = factor[v]; ga.bias[v] = bias[v];
    }
    sa.n_var = n_var; sa.R = m->R; sa.reduced = m->identity ? nullptr : m->dreduced.p;
    sa.east_west = m->east_west; sa.lat = m->dlat.p; sa.lon = m->dlon.p; sa.map = m->map; sa.Re = NXS_MAPX_RE_KM * 1000.;
    sa.rotate = m->rotate; sa.c = m->c; sa.s = m->s; sa.cs = m->dcs.p; sa.sn = m->dsn.p;
    sa.stage = m->dstage.p;
    ga.stage = m->dstage.p; ga.R = m->R; ga.N = m->N; ga.get = (flags & NXS_NODEMAP_GET) ? 1 : 0;
    hipLaunchKernelGGL(nodemap::k_nodemap_source, dim3((unsigned)((m->R + 255) / 256)), dim3(256), 0, st, sa);
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    const int *v0 = m->v0.p, *v1 = m->v1.p, *v2 = m->v2.p;
    const double *a0 = m->a0.p, *a1 = m->a1.p, *a2 = m->a2.p;
#define NXS_GATHER(NV) case NV: hipLaunchKernelGGL((nodemap::k_nodemap_gather<NV>), grid, block, 0, st, ga, v0, v1, v2, a0, a1, a2); break;
    switch (n_var) { NXS_GATHER(1) NXS_GATHER(2) NXS_GATHER(3) NXS_GATHER(4) }
#undef NXS_GATHER
    m->last_n_var = n_var;
    if (hipGetLastError() != hipSuccess) return fail(NXS_ERR_HIP, "nodemap_receive_rows: kernel launch failed");
    if (stream && out_dev) return NXS_OK;   // asynchronous on the caller's stream
    if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "nodemap_receive_rows: kernels failed: %s", hipGetErrorString(hipGetLastError()));
    if (!out_dev)
        for (int v = 0; v < n_var; ++v)
            if (copy_sync(out_rows[v], dout.p + (size_t)v * N, N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_receive_rows"); }

// test door: loaded_data of the last receive, [n_var][R]
extern "C" int nxs_nodemap_debug_source(nxs_nodemap *m, double *out, int32_t n_var) try {
    if (!m || !out) return fail(NXS_ERR_INVALID, "nodemap_debug_source: NULL argument");
    if (!m->have_source || m->last_n_var < 1) return fail(NXS_ERR_STATE, "nodemap_debug_source: no nxs_nodemap_receive_rows on this source yet");
    if (n_var < 1 || n_var > m->last_n_var) return fail(NXS_ERR_INVALID, "nodemap_debug_source: n_var = %d, the last receive had %d", n_var, m->last_n_var);
    if (hipSetDevice(m->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail(NXS_ERR_HIP, "hipDeviceSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
    if (copy_sync(out, m->dstage.p, (size_t)n_var * m->R * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_debug_source"); }

// One loadDataset of a FromMeshToMesh2dx dataset (externaldata.cpp:886-931, 944-1288, 1334-1383, 1442-1448): k_nodemap_load, k_nodemap_cols_gather on `stream`
extern "C" int nxs_nodemap_load_rows(nxs_nodemap *m, const nxs_nodemap_load *l, double *const *out_rows, int32_t flags, void *stream) try {
    if (!m || !l || !out_rows) return fail(NXS_ERR_INVALID, "nodemap_load_rows: NULL argument");
    if (!l->fields) return fail(NXS_ERR_INVALID, "nodemap_load_rows: NULL argument (fields)");
    if (l->n_var < 1 || l->n_var > nodemap::kMaxVar) return fail(NXS_ERR_INVALID, "nodemap_load_rows: n_var = %d (1 .. %d)", l->n_var, nodemap::kMaxVar);
    if (l->n_step < 1 || l->n_step > 2) return fail(NXS_ERR_INVALID, "nodemap_load_rows: n_step = %d (1 or 2)", l->n_step);
    const int n_var = l->n_var, ncols = l->n_step * l->n_var;
    static_assert(NXS_NODEMAP_MAX_LOAD == nodemap::kMaxLoad && nodemap::kMaxLoad == 2 * nodemap::kMaxVar, "columns: variables x forcing steps");
    nodemap::ColsArgs ga{};
    int kept = 0;
    for (int c = 0; c < ncols; ++c) {
        if (!l->fields[c]) return fail(NXS_ERR_INVALID, "nodemap_load_rows: field %d (forcing step %d, variable %d) is NULL", c, c / n_var, c % n_var);
        if (!std::isfinite(l->scale_factor[c]) || !std::isfinite(l->add_offset[c]) || !std::isfinite(l->a[c]) || !std::isfinite(l->b[c]))
            return fail(NXS_ERR_INVALID, "nodemap_load_rows: scale_factor, add_offset, a or b of column %d is not finite", c);
        if (out_rows[c]) ga.col[kept++] = c;   // skipped columns are compacted away
    }
    if (kept == 0) return fail(NXS_ERR_INVALID, "nodemap_load_rows: every column is skipped");
    nodemap::LoadArgs sa{};
    {
        int used[nodemap::kMaxVar] = {0, 0, 0, 0};
        for (int v = 0; v < n_var; ++v) {
            const int w = l->pairs[v];
            if (w < 0) continue;
            if (w >= n_var || w == v) return fail(NXS_ERR_INVALID, "nodemap_load_rows: pairs[%d] = %d is not another variable (0 .. %d)", v, w, n_var - 1);
            if (used[v] || used[w]) return fail(NXS_ERR_INVALID, "nodemap_load_rows: variable %d is named by two pairs", used[v] ? v : w);
            used[v] = used[w] = 1;
            sa.j0[sa.npairs] = v; sa.j1[sa.npairs] = w; ++sa.npairs;   // (four variables hold at most two pairs)
        }
    }
    if (!m->have_source) return fail(NXS_ERR_STATE, "nodemap_load_rows: before nxs_nodemap_set_source");
    if (flags & ~(NXS_REGRID_IN_DEVICE | NXS_REGRID_OUT_DEVICE)) return fail(NXS_ERR_INVALID, "nodemap_load_rows: flags = 0x%x (NXS_REGRID_IN_DEVICE, NXS_REGRID_OUT_DEVICE)", flags);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the node map has no CPU path");
    if (hipSetDevice(m->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    const bool in_dev = flags & NXS_REGRID_IN_DEVICE, out_dev = flags & NXS_REGRID_OUT_DEVICE;
    const hipStream_t st = stream ? (hipStream_t)stream : S();
    const size_t G = (size_t)m->G, N = (size_t)m->N, R = (size_t)m->R;
    if (m->load_cap < (size_t)ncols * R) {   // the first load, or the first with this many columns
        if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "hipStreamSynchronize failed");   // (an earlier load may still read the buffer)
        m->last_load_cols = 0;
        if (m->dload.alloc((size_t)ncols * R)) { m->load_cap = 0; return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError())); }
        m->load_cap = (size_t)ncols * R;
    }
    if (!in_dev) {   // the fields go up on the same stream; the host arrays are the caller's again on return
        if (m->fields_cap < (size_t)ncols * G) {
            if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "hipStreamSynchronize failed");   // (an earlier load or receive may still read the buffer)
            if (m->dfields.alloc((size_t)ncols * G)) { m->fields_cap = 0; return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError())); }
            m->fields_cap = (size_t)ncols * G;
        }
        for (int c = 0; c < ncols; ++c)
            if (hipMemcpyAsync(m->dfields.p + (size_t)c * G, l->fields[c], G * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
    DevBuf<double> dout;
    if (!out_dev && dout.alloc((size_t)kept * N)) return fail(NXS_ERR_HIP, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
    for (int c = 0; c < ncols; ++c) {
        sa.field[c] = in_dev ? l->fields[c] : m->dfields.p + (size_t)c * G;
        sa.scale_factor[c] = l->scale_factor[c]; sa.add_offset[c] = l->add_offset[c]; sa.a[c] = l->a[c]; sa.b[c] = l->b[c];
    }
    for (int k = 0; k < kept; ++k) ga.out[k] = out_dev ? out_rows[ga.col[k]] : dout.p + (size_t)k * N;
    sa.n_var = n_var; sa.n_step = l->n_step; sa.R = m->R; sa.reduced = m->identity ? nullptr : m->dreduced.p;
    sa.east_west = m->east_west; sa.lat = m->dlat.p; sa.lon = m->dlon.p; sa.map = m->map; sa.Re = NXS_MAPX_RE_KM * 1000.;
    sa.rotate = m->rotate; sa.c = m->c; sa.s = m->s; sa.cs = m->dcs.p; sa.sn = m->dsn.p;
    sa.stage = m->dload.p;
    ga.stage = m->dload.p; ga.R = m->R; ga.N = m->N;
    hipLaunchKernelGGL(nodemap::k_nodemap_load, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, sa);
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    const int *v0 = m->v0.p, *v1 = m->v1.p, *v2 = m->v2.p;
    const double *a0 = m->a0.p, *a1 = m->a1.p, *a2 = m->a2.p;
#define NXS_GATHER(NC) case NC: hipLaunchKernelGGL((nodemap::k_nodemap_cols_gather<NC>), grid, block, 0, st, ga, v0, v1, v2, a0, a1, a2); break;
    switch (kept) { NXS_GATHER(1) NXS_GATHER(2) NXS_GATHER(3) NXS_GATHER(4) NXS_GATHER(5) NXS_GATHER(6) NXS_GATHER(7) NXS_GATHER(8) }
#undef NXS_GATHER
    m->last_load_cols = ncols;
    if (hipGetLastError() != hipSuccess) return fail(NXS_ERR_HIP, "nodemap_load_rows: kernel launch failed");
    if (stream && out_dev) return NXS_OK;   // asynchronous on the caller's stream
    if (hipStreamSynchronize(st) != hipSuccess) return fail(NXS_ERR_HIP, "nodemap_load_rows: kernels failed: %s", hipGetErrorString(hipGetLastError()));
    if (!out_dev)
        for (int k = 0; k < kept; ++k)
            if (copy_sync(out_rows[ga.col[k]], dout.p + (size_t)k * N, N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_load_rows"); }

// test door: loaded_data of the last load, [n_cols][R]
extern "C" int nxs_nodemap_debug_load(nxs_nodemap *m, double *out, int32_t n_cols) try {
    if (!m || !out) return fail(NXS_ERR_INVALID, "nodemap_debug_load: NULL argument");
    if (!m->have_source || m->last_load_cols < 1) return fail(NXS_ERR_STATE, "nodemap_debug_load: no nxs_nodemap_load_rows on this source yet");
    if (n_cols < 1 || n_cols > m->last_load_cols) return fail(NXS_ERR_INVALID, "nodemap_debug_load: n_cols = %d, the last load had %d", n_cols, m->last_load_cols);
    if (hipSetDevice(m->device) != hipSuccess) return fail(NXS_ERR_HIP, "hipSetDevice failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail(NXS_ERR_HIP, "hipDeviceSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
    if (copy_sync(out, m->dload.p, (size_t)n_cols * m->R * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_nodemap_debug_load"); }

// ---------------------------------------------------------------------------------------------------------
// Structured grid -> mesh nodes: the forcing ingest (InterpFromGridToMeshx, called at externaldata.cpp:1436)
// ---------------------------------------------------------------------------------------------------------
namespace {

#include "nxs_grid_to_mesh_body.inl"   // G2M, find_interval, grid_to_mesh_point: shared with k_thermo_forcing_ingest (nxs_thermo_forcing_kernels.inl)

struct G2MInterleaved {   // column j of node i goes to out[i][j]
    double *o;
    __device__ __forceinline__ bool wants(int) const { return true; }
    __device__ __forceinline__ void put(int j, double v) const { o[j] = v; }
};

__global__ void __launch_bounds__(256) k_grid_to_mesh(G2M g, const double *__restrict__ data, const double *__restrict__ xm, const double *__restrict__ ym,
                                                      double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.nods) return;
    grid_to_mesh_point(g, data, xm[i], ym[i], G2MInterleaved{out + (size_t)i * g.N_data});
}

}  // namespace

extern "C" int nxs_interp_grid_to_mesh(double *data_mesh, const double *x_in, int32_t x_rows, const double *y_in, int32_t y_rows, const double *data,
                                       int32_t M, int32_t N, int32_t N_data, const double *x_mesh, const double *y_mesh, int32_t nods,
                                       double default_value, int32_t interp, int32_t row_major, int32_t device, double *kernel_ms) try {
    if (!data_mesh || !x_in || !y_in || !data || !x_mesh || !y_mesh) return fail(NXS_ERR_INVALID, "NULL argument");
    if ((M < 2) || (N < 2) || (nods <= 0) || N_data < 1) return fail(NXS_ERR_INVALID, "nothing to be done according to the dimensions of input matrices and vectors.");
    if (interp != NXS_INTERP_TRIANGLE && interp != NXS_INTERP_BILINEAR && interp != NXS_INTERP_NEAREST) return fail(NXS_ERR_INVALID, "Interpolation %d not supported yet", interp);
    std::vector<double> x(N), y(M);
    if (!g2m_centres(x_in, x_rows, y_in, y_rows, M, N, x.data(), y.data()))  // contours of the pixels given: the centres are taken (:44-53)
        return fail(NXS_ERR_INVALID, "x and y vectors length should be 1 or 0 more than data number of rows.");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the interpolation has no CPU path");
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return fail(NXS_ERR_INVALID, "bad device %d", device);
    DevBuf<double> dx, dy, dd, dxm, dym, dout;
    if (dx.upload(x.data(), N) || dy.upload(y.data(), M) || dd.upload(data, (size_t)M * N * N_data) || dxm.upload(x_mesh, nods) || dym.upload(y_mesh, nods) ||
        dout.alloc((size_t)nods * N_data))
        return fail(NXS_ERR_HIP, "device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    G2M g{dx.p, dy.p, N, M, M, N, N_data, nods, interp, row_major != 0, g2m_monotone(x.data(), N), g2m_monotone(y.data(), M), default_value};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, S());
    hipLaunchKernelGGL(k_grid_to_mesh, dim3((nods + 255) / 256), dim3(256), 0, S(), g, (const double *)dd.p, (const double *)dxm.p, (const double *)dym.p, dout.p);
    (void)hipEventRecord(e1, S());
    hipError_t err = hipStreamSynchronize(S());
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(NXS_ERR_HIP, "grid-to-mesh kernel failed: %s", hipGetErrorString(err));
    if (kernel_ms) *kernel_ms = ms;
    if (copy_sync(data_mesh, dout.p, (size_t)nods * N_data * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(NXS_ERR_HIP, "copy back failed");
    return NXS_OK;
} catch (...) { return entry_caught("nxs_interp_grid_to_mesh"); }

// ---------------------------------------------------------------------------------------------------------
// The drifters of a dynamics handle (nxs_dyn_drifters_*): kernels that share locate() with k_interp, and the locator built from device coordinates
// ---------------------------------------------------------------------------------------------------------
#include "nxs_drifters.inl"
// The Moorings means on a loaded grid (nxs_dyn_means_points_*): one more consumer of locate() and of the drifters' locators
#include "nxs_means_points_kernels.inl"
