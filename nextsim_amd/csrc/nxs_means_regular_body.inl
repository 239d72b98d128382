// nxs_means_regular_body.inl -- GridOutput::updateGridMean() on the REGULAR grid (nxs_dyn_means_regular_update, include/nxs_dyn.h) as two bodies:
//   element_hits  the element loop of InterpFromMeshToGridx for ONE element: its box, the :111 test, the window of :120-130, and for every grid point of the
//                 window that the triangle holds, emit(grid index).  The reference's loop overwrites, so the LAST element in ascending order wins a point; the
//                 kernel emits into an integer maximum, which is the same thing in any order.
//   point         ONE grid point whose winner is known: the area coordinates again (the SAME function, so the same bits), the P0 and P1 values with the NaN
//                 rule of :175, rotateVectors, the product with the proc mask, the accumulation in grid order, the ice-mask rule.
// __host__ __device__ text, no device intrinsic: k_means_regular_hits / k_means_regular_gather (nxs_means_regular_kernels.inl) call it per thread, and
// tests/means_regular_host_kernel.cpp compiles the same text with g++ -O2 -ffp-contract=off and holds it against the fixture the real contrib/bamg wrote.
//
// Reference: contrib/bamg/src/InterpFromMeshToGridx.cpp:78, 88, 94-181; model/gridoutput.cpp:360-378 (setProcMask), :387-415 (updateGridMean), :486-505 and :511-538
// (updateGridMeanWorker, M_is_regular_grid), :578-623 (rotateVectors).  bamg's "nrows" is M_ncols (along x) and its "ncols" is M_nrows (along y): the bamg index of
// the point (i, j) is b = i * M_nrows + j, its grid index g = i + M_ncols * j.  Every sum and product below is one the reference makes, in its operand order (that
// of k_mesh_to_grid, nxs_interp.hip); the build forbids contraction.
//
// rotateVectors (:595-622) walks interp_out in BAMG order and indexes M_grid.gridLON by the same number, although initRegularGrid filled gridLON in GRID order
// (:199-213): the point (i, j) is rotated by the longitude of whichever point has the grid index b.  That is restated as it stands: cosang / sinang are indexed by b.
//
// What follows the interpolation (rotateVectors on a per-point row, the product with the proc mask, the ice-mask rule) is the loaded grid's text,
// nxs_means_points_body.inl, called with the index each step uses.
#ifndef NXS_MEANS_REGULAR_BODY_INL
#define NXS_MEANS_REGULAR_BODY_INL

#include "nxs_means_points_body.inl"

namespace nxs_mr {

struct Args {   // travels to the kernels by value
    nxs_mp::Args m;                       // G = ncols * nrows, the lists, the pairs, cosang / sinang [G] BY BAMG INDEX, both accumulator sets (gx, gy unused)
    int ncols, nrows;                     // M_ncols (along x), M_nrows (along y)
    int Ne, Nn;
    double spacing;                       // M_mooring_spacing > 0: neither axis is flipped
    const double *xg, *yg;                // [ncols], [nrows] x_grid, y_grid as InterpFromMeshToGridx.cpp:78, 88 builds them
    const int *t0, *t1, *t2;              // [Ne] 0-based
    const double *x0, *y0;                // [Nn] the mesh at rest
    const double *UM;                     // [2 Nn] M_UM; NULL: the mesh at rest (setLSM)
    int *hit;                             // [G] by grid index: the winning element, -1: none
};

struct Tri { double x1, y1, x2, y2, x3, y3; };

// coordX / coordY of gridoutput.cpp:445-446 for the three vertices of element n
__host__ __device__ inline Tri vertices(const Args &a, int n) {
    const int i0 = a.t0[n], i1 = a.t1[n], i2 = a.t2[n];
    Tri t{a.x0[i0], a.y0[i0], a.x0[i1], a.y0[i1], a.x0[i2], a.y0[i2]};
    if (a.UM) {
        t.x1 = t.x1 + a.UM[i0]; t.y1 = t.y1 + a.UM[(size_t)i0 + a.Nn];
        t.x2 = t.x2 + a.UM[i1]; t.y2 = t.y2 + a.UM[(size_t)i1 + a.Nn];
        t.x3 = t.x3 + a.UM[i2]; t.y3 = t.y3 + a.UM[(size_t)i2 + a.Nn];
    }
    return t;
}

struct Box { double xmin, xmax, ymin, ymax; };
__host__ __device__ inline Box box_of(const Tri &t) {   // :101-108
    Box b{t.x1, t.x1, t.y1, t.y1};
    if (t.x2 < b.xmin) b.xmin = t.x2; if (t.x2 > b.xmax) b.xmax = t.x2; if (t.y2 < b.ymin) b.ymin = t.y2; if (t.y2 > b.ymax) b.ymax = t.y2;
    if (t.x3 < b.xmin) b.xmin = t.x3; if (t.x3 > b.xmax) b.xmax = t.x3; if (t.y3 < b.ymin) b.ymin = t.y3; if (t.y3 > b.ymax) b.ymax = t.y3;
    return b;
}

// :135-137
__host__ __device__ inline double area_of(const Tri &t) { return t.x2 * t.y3 - t.y2 * t.x3 + t.x1 * t.y2 - t.y1 * t.x2 + t.x3 * t.y1 - t.y3 * t.x1; }

// :143, :148, :152-161 -- does the triangle hold (xg, yg)?  ar[] = area_1, area_2, area_3.  The ONE copy of the search's arithmetic: both bodies call it.
__host__ __device__ inline bool holds(const Tri &t, const Box &b, double area, double xg, double yg, double ar[3]) {
    if ((xg > b.xmax) || (xg < b.xmin) || (yg > b.ymax) || (yg < b.ymin)) return false;
    ar[0] = ((xg - t.x3) * (t.y2 - t.y3) - (yg - t.y3) * (t.x2 - t.x3)) / area;
    ar[1] = ((t.x1 - t.x3) * (yg - t.y3) - (t.y1 - t.y3) * (xg - t.x3)) / area;
    ar[2] = 1 - ar[0] - ar[1];
    return ar[0] > -10e-12 && ar[1] > -10e-12 && ar[2] > -10e-12;
}

// (int)floor(.) / (int)ceil(.) of :120-130 wherever the reference's conversion is defined; a quotient beyond int (a triangle far larger than the grid) is clamped
// in front of the conversion, which the max / min of the window does anyway, and a NaN (a NaN coordinate: no point can be held) gives an empty window
__host__ __device__ inline int to_index(double f) { return f >= -2e9 ? (int)(f < 2e9 ? f : 2e9) : -2000000000; }

template <class Emit>
__host__ __device__ inline void element_hits(const Args &a, int n, Emit emit) {
    const Tri t = vertices(a, n);
    const Box b = box_of(t);
    const double x_grid_min = a.xg[0], x_grid_max = a.xg[a.ncols - 1], y_grid_min = a.yg[0], y_grid_max = a.yg[a.nrows - 1];
    if ((b.xmin > x_grid_max) || (b.xmax < x_grid_min) || (b.ymin > y_grid_max) || (b.ymax < y_grid_min)) return;   // :111
    int i1 = to_index(floor((b.xmin - x_grid_min) / a.spacing)) - 1, i2 = to_index(ceil((b.xmax - x_grid_min) / a.spacing));   // :120-121
    int j1 = to_index(floor((b.ymin - y_grid_min) / a.spacing)) - 1, j2 = to_index(ceil((b.ymax - y_grid_min) / a.spacing));   // :129-130
    if (i1 < 0) i1 = 0; if (i2 > a.ncols - 1) i2 = a.ncols - 1;
    if (j1 < 0) j1 = 0; if (j2 > a.nrows - 1) j2 = a.nrows - 1;
    const double area = area_of(t);
    double ar[3];
    for (int i = i1; i <= i2; ++i) {
        const double xg = a.xg[i];
        if ((xg > b.xmax) || (xg < b.xmin)) continue;   // :143
        for (int j = j1; j <= j2; ++j)
            if (holds(t, b, area, xg, a.yg[j], ar)) emit(i + a.ncols * j);
    }
}

// the elemental leg: data_mesh[N_data * n + k], a NaN becomes the default 0. (:173-175), 0. where nothing holds the point; gridoutput.cpp:535
__host__ __device__ inline void elemental(const Args &a, int g, int n) {
    const double *row = a.m.el + (size_t)(n >= 0 ? n : 0) * a.m.n_el;
    for (int nv = 0; nv < a.m.n_el; ++nv) {
        double value = n >= 0 ? row[nv] : 0.;
        if (value != value) value = 0.;
        a.m.grid_el[(size_t)nv * a.m.G + g] += value;
    }
}

// the nodal leg: :167-169 and :175 into the point's interp_out row v[nv * stride]
__host__ __device__ inline void nodal_interp(const Args &a, int i, int j, int n, double *v, int stride) {
    if (n < 0) {
        for (int nv = 0; nv < a.m.n_nod; ++nv) v[nv * stride] = 0.;
        return;
    }
    const Tri t = vertices(a, n);
    double ar[3] = {0., 0., 0.};
    (void)holds(t, box_of(t), area_of(t), a.xg[i], a.yg[j], ar);
    const double *r0 = a.m.nod + (size_t)a.m.n_nod * a.t0[n], *r1 = a.m.nod + (size_t)a.m.n_nod * a.t1[n], *r2 = a.m.nod + (size_t)a.m.n_nod * a.t2[n];
    for (int nv = 0; nv < a.m.n_nod; ++nv) {
        double value = ar[0] * r0[nv];
        value += ar[1] * r1[nv];
        value += ar[2] * r2[nv];
        if (value != value) value = 0.;
        v[nv * stride] = value;
    }
}

// one grid point, in grid order; v: its interp_out row (LDS with stride 256 on the device, a plain array on the host)
__host__ __device__ inline void point(const Args &a, int g, double *v, int stride) {
    const int i = g % a.ncols, j = g / a.ncols;
    const int n = a.hit[g];
    elemental(a, g, n);
    if (a.m.n_nod > 0) {
        nodal_interp(a, i, j, n, v, stride);
        nxs_mp::rotate(a.m, i * a.nrows + j, v, stride);                                  // by BAMG index, gridLON's included
        nxs_mp::nodal_add(a.m, g, (n >= 0 && n < a.m.Neo) ? 1. : 0., v, stride);          // setProcMask: 1. in an owned element
    }
    nxs_mp::ice_mask(a.m, g);
}

}  // namespace nxs_mr
#endif
