// nxs_means_points_body.inl -- what updateGridMean() does at ONE point of a loaded grid once the point is located (nxs_dyn_means_points_update, include/nxs_dyn.h):
// the gather of both accumulator rows, rotateVectors, the product with the proc mask, the accumulation into data_grid, the ice-mask rule.
// __host__ __device__ text, no device intrinsic: k_means_points (nxs_means_points_kernels.inl) calls it per thread, and tests/means_points_host_kernel.cpp compiles
// the same text with g++ -O2 -ffp-contract=off and holds it against the fixture the real contrib/bamg wrote.
//
// Reference: model/gridoutput.cpp:387-415 (updateGridMean), :470-485 and :511-545 (updateGridMeanWorker, M_grid.loaded, not conservative), :578-623 (rotateVectors),
// contrib/bamg/src/InterpFromMeshToMesh2dx.cpp:113-116, 151-170.  Every sum and product below is one the reference makes, in its operand order; the build forbids
// contraction, so a * b + c stays two roundings.
//
// interp_out of the nodal leg is a per-point row of n_nod doubles that rotateVectors indexes by the pairs' column numbers: it lives at v[nv * stride] -- a
// workgroup's LDS with stride 256 on the device (a per-thread array indexed at run time would go to scratch memory), a plain array with stride 1 on the host.
#ifndef NXS_MEANS_POINTS_BODY_INL
#define NXS_MEANS_POINTS_BODY_INL

namespace nxs_mp {

constexpr int MAX_VARS = 24;    // NXS_MEANS_MAX_VARS
constexpr int MAX_PAIRS = 12;   // NXS_MEANS_MAX_PAIRS

struct Args {   // travels to the kernel by value
    int G, n_el, n_nod, n_pairs;
    int ice_col;                          // the elemental column of NXS_MEANS_ICE_MASK, -1: no rule
    int Neo;                              // owned elements come first: proc_mask = 1. below it
    unsigned mask_el, mask_nod;           // Variable::mask, bit nv
    unsigned char first[MAX_PAIRS], second[MAX_PAIRS];
    double miss_val;
    const double *gx, *gy;                // [G]
    const double *cosang, *sinang;        // [G]; NULL: NXS_MEANS_ROTATE_NONE
    const double *el, *nod;               // the mesh accumulators [Ne][n_el], [Nn][n_nod]
    double *grid_el, *grid_nod;           // data_grid [n_el][G], [n_nod][G]
};

// the elemental leg, P0 (InterpFromMeshToMesh2dx.cpp:163-170; default 0. when no element holds the point), gridoutput.cpp:545
__host__ __device__ inline void elemental(const Args &a, int j, int it) {
    const double *row = a.el + (size_t)(it >= 0 ? it : 0) * a.n_el;
    for (int nv = 0; nv < a.n_el; ++nv) {
        const double value = it >= 0 ? row[nv] : 0.;
        a.grid_el[(size_t)nv * a.G + j] += value;
    }
}

// the nodal leg, P1 (InterpFromMeshToMesh2dx.cpp:113-116, 157-159); dd = the three integer area coordinates of the point in triangle (i0, i1, i2)
__host__ __device__ inline void nodal_interp(const Args &a, int it, int i0, int i1, int i2, const long long dd[3], double *v, int stride) {
    if (it < 0) {
        for (int nv = 0; nv < a.n_nod; ++nv) v[nv * stride] = 0.;
        return;
    }
    const long long det = dd[0] + dd[1] + dd[2];
    const double a0 = (double)dd[0] / det, a1 = (double)dd[1] / det, a2 = (double)dd[2] / det;
    const double *r0 = a.nod + (size_t)a.n_nod * i0, *r1 = a.nod + (size_t)a.n_nod * i1, *r2 = a.nod + (size_t)a.n_nod * i2;
    for (int nv = 0; nv < a.n_nod; ++nv) v[nv * stride] = a0 * r0[nv] + a1 * r1[nv] + a2 * r2[nv];
}

// rotateVectors for every pair, in list order (gridoutput.cpp:513-514, 593-622)
__host__ __device__ inline void rotate(const Args &a, int j, double *v, int stride) {
    if (!a.cosang) return;
    const double cosang = a.cosang[j], sinang = a.sinang[j];
    for (int k = 0; k < a.n_pairs; ++k) {
        const int first = a.first[k] * stride, second = a.second[k] * stride;
        if (v[first] == a.miss_val) continue;
        const double u = cosang * v[first] - sinang * v[second];
        const double w = sinang * v[first] + cosang * v[second];
        v[first] = u;
        v[second] = w;
    }
}

// data_grid[nv][j] += interp_out[nb_var * j + nv] * M_proc_mask[j] (gridoutput.cpp:543): the product is made even where the mask is 0 (a NaN stays a NaN)
__host__ __device__ inline void nodal_add(const Args &a, int j, double proc_mask, const double *v, int stride) {
    for (int nv = 0; nv < a.n_nod; ++nv) a.grid_nod[(size_t)nv * a.G + j] += v[nv * stride] * proc_mask;
}

// the ice-mask rule on the accumulated values (gridoutput.cpp:404-414): nodal variables first, then the elemental ones in their order
__host__ __device__ inline void ice_mask(const Args &a, int j) {
    if (a.ice_col < 0) return;
    const double *ice = a.grid_el + (size_t)a.ice_col * a.G + j;   // (read again for every variable, as the reference does: the column may be masked itself)
    for (int nv = 0; nv < a.n_nod; ++nv)
        if (a.mask_nod >> nv & 1u) {
            double *g = a.grid_nod + (size_t)nv * a.G + j;
            if (*ice <= 0. && *g != a.miss_val) *g = 0.;
        }
    for (int nv = 0; nv < a.n_el; ++nv)
        if (a.mask_el >> nv & 1u) {
            double *g = a.grid_el + (size_t)nv * a.G + j;
            if (*ice <= 0. && *g != a.miss_val) *g = 0.;
        }
}

// one grid point, located: it = the triangle (-1: none, or outside the box), (i0, i1, i2) its vertices, dd its integer area coordinates
__host__ __device__ inline void point(const Args &a, int j, int it, int i0, int i1, int i2, const long long dd[3], double *v, int stride) {
    elemental(a, j, it);
    if (a.n_nod > 0) {
        nodal_interp(a, it, i0, i1, i2, dd, v, stride);
        rotate(a, j, v, stride);
        nodal_add(a, j, (it >= 0 && it < a.Neo) ? 1. : 0., v, stride);
    }
    ice_mask(a, j);
}

}  // namespace nxs_mp
#endif
