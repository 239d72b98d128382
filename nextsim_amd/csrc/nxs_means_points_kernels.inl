// nxs_means_points_kernels.inl -- updateGridMean() on a loaded grid as ONE launch (nxs_dyn_means_points_update) and setLSM on the mesh at rest
// (nxs_dyn_means_points_lsm).  Textually included by nxs_interp.hip behind nxs_drifters.inl: the kernels share locate() -- which exists once -- and the two
// locators of nxs_drifters::State with the drifters; the interface is nxs_drifters.hpp, the host side nxs_means_points.inl (nxs_dyn.hip).
//
// Reference: model/gridoutput.cpp:387-415, 470-485, 511-545, 558-574, 578-623; contrib/bamg/src/InterpFromMeshToMesh2dx.cpp:92, 113-170.  The reference
// interpolates three times (elemental variables, nodal variables, proc mask) with isdefault = true and default 0.; the mesh and the points are the same each
// time, so one location serves all three.  What follows the location is nxs_means_points_body.inl.
//
// One thread per grid point, 256 per block.  The accumulator rows are interleaved ([Ne][n_el], [Nn][n_nod]): a thread reads n_el consecutive doubles of one
// element and three runs of n_nod consecutive doubles; the grid rows are [var][G], so neighbouring threads read-modify-write neighbouring addresses.  The nodal
// leg's interp_out row is staged in dynamic LDS ([n_nod][256], one column per thread: conflict-free), because rotateVectors indexes it by run-time column numbers.

namespace nxs_drifters {
namespace {

__global__ void __launch_bounds__(256) k_means_points(InterpDev d, nxs_mp::Args a) {
    extern __shared__ double mp_interp_out[];   // [n_nod][256]
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.G) return;
    const double px = a.gx[j], py = a.gy[j];
    long long dd[3] = {0, 0, 0}, Bx, By;
    int it = -1, i0 = 0, i1 = 0, i2 = 0;
    if (!(px < d.xmin || px > d.xmax || py < d.ymin || py > d.ymax)) it = locate(d, px, py, dd, Bx, By);   // InterpFromMeshToMesh2dx.cpp:92
    if (it >= 0) { i0 = d.t0[it]; i1 = d.t1[it]; i2 = d.t2[it]; }
    nxs_mp::point(a, j, it, i0, i1, i2, dd, mp_interp_out + threadIdx.x, 256);
}

// setLSM: a column of ones on every triangle, ghosts included, sampled with default 0. in the mesh at rest, then the conversion to int (gridoutput.cpp:563-573)
__global__ void __launch_bounds__(256) k_means_points_lsm(InterpDev d, int G, const double *__restrict__ gx, const double *__restrict__ gy, int *__restrict__ lsm) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= G) return;
    const double px = gx[j], py = gy[j];
    long long dd[3] = {0, 0, 0}, Bx, By;
    int it = -1;
    if (!(px < d.xmin || px > d.xmax || py < d.ymin || py > d.ymax)) it = locate(d, px, py, dd, Bx, By);
    lsm[j] = it >= 0 ? 1 : 0;
}

#define MPCHK(call)                                                                                                      \
    do {                                                                                                                 \
        hipError_t _e = (call);                                                                                          \
        if (_e != hipSuccess) { err = std::string(#call " failed: ") + hipGetErrorString(_e); return NXS_ERR_HIP; }       \
    } while (0)

}  // namespace

int means_points_update(State *s, hipStream_t st, const MeshView &m, const double *UM, const nxs_mp::Args &a, std::string &err) {
    if (a.G <= 0) return NXS_OK;
    const unsigned builds = s->builds;
    if (int rc = ensure_locator(s, st, m, UM, nullptr, err)) return rc;
    s->mp_ms[0] = s->builds != builds ? s->ms[0] : 0.;
    {
        Timed tm(s, st, 4);
        hipLaunchKernelGGL(k_means_points, dim3(grid_blocks(a.G)), dim3(256), (size_t)256 * a.n_nod * sizeof(double), st, s->loc[UM ? 1 : 0].d, a);
        MPCHK(hipGetLastError());
    }
    s->mp_ms[1] = s->ms[4];
    return NXS_OK;
}

int means_points_lsm(State *s, hipStream_t st, const MeshView &m, int G, const double *gx, const double *gy, int *lsm, std::string &err) {
    if (G <= 0) return NXS_OK;
    if (int rc = ensure_locator(s, st, m, nullptr, nullptr, err)) return rc;
    hipLaunchKernelGGL(k_means_points_lsm, dim3(grid_blocks(G)), dim3(256), 0, st, s->loc[0].d, G, gx, gy, lsm);
    MPCHK(hipGetLastError());
    return NXS_OK;
}

bool means_points_timing(const State *s, double ms[2]) {
    ms[0] = s->mp_ms[0]; ms[1] = s->mp_ms[1];
    return s->timed;
}

#undef MPCHK

}  // namespace nxs_drifters
