// nxs_nodemap_load_kernels.inl -- one loadDataset of a dataset interpolated with InterpFromMeshToMesh2dx, through the weights of a node map (include/nxs_interp.h,
// nxs_nodemap_load_rows).  Textually included by nxs_interp.hip inside its unnamed namespace, behind nxs_nodemap_kernels.inl (whose enums, east/north include and
// namespace it continues).  externaldata.cpp = model/externaldata.cpp, bamg = contrib/bamg/src.
//   k_nodemap_load        one thread per reduced source point.  Per column c = fstep*n_var + j (loadDataset's order, externaldata.cpp:1378):
//                d = field[c][reduced[i]]; d = (d*scale_factor + add_offset)*a + b as four separately rounded operations (:908); NaN becomes 0. (:923-927; the
//                wave-direction exception is not built).  Then transformData per forcing step and pair on the point's own two entries: the east/north branch
//                (nf_east_north_point, nxs_east_north_body.inl), then the uniform (:1246-1261) or the per-point rotation (:1263-1281), the statements of
//                k_nodemap_source.  ONE loop over (forcing step, pair), not unrolled: the east/north body is carried once.  Rows [n_step*n_var][R] of the map's
//                load staging buffer.
//   k_nodemap_cols_gather<NC>   InterpFromMeshToMesh2dx.cpp:157-159, one thread per target: three vertices and three weights loaded once, per KEPT column
//                a0*d[v0] + a1*d[v1] + a2*d[v2] left to right, stored to that column's own [N] row (the host compacts skipped columns away: col[k] is the staged
//                column of kept column k).  No factor / bias: ExternalData::get is the time blend's.  No atomics, no LDS, no scratch.
// The bodies compile for the host (tests/mesh_forcing_host_kernel.cpp defines the HIP qualifiers away).  The build is uncontracted (-ffp-contract=off).

namespace nodemap {

enum { kMaxLoad = 8 };   // NXS_NODEMAP_MAX_LOAD: up to kMaxVar variables x two forcing steps

struct LoadArgs {
    const double *field[kMaxLoad];  // [G] each: data_in_tmp of column fstep*n_var + j, as read from the file
    double scale_factor[kMaxLoad], add_offset[kMaxLoad], a[kMaxLoad], b[kMaxLoad];
    int n_var, n_step, R;
    const int *reduced;             // [R] grid.reduced_nodes_ind, NULL = the identity
    int npairs, j0[kMaxPairs], j1[kMaxPairs];   // variables; applied in every forcing step
    int east_west;
    const double *lat, *lon;        // [R] degrees, read only under east_west
    nxs_mapx_polar map;
    double Re;                      // mapx_Re_km*1000.
    int rotate;                     // ROTATE_*
    double c, s;                    // ROTATE_UNIFORM: cos / sin(-rotation_angle)
    const double *cs, *sn;          // ROTATE_GRID_THETA: [R] cos / sin(rotation - theta[i])
    double *stage;                  // [n_step*n_var][R] loaded_data
};

// externaldata.cpp:908, 922-927 on one entry
__device__ __forceinline__ double nodemap_load_value(double d, double scale_factor, double add_offset, double a, double b) {
    d = d * scale_factor;
    d = d + add_offset;
    d = d * a;
    d = d + b;
    return d != d ? 0. : d;
}

__global__ void __launch_bounds__(256) k_nodemap_load(LoadArgs s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.R) return;
    const int g = s.reduced ? s.reduced[i] : i;
    const size_t R = (size_t)s.R;
    const int ncols = s.n_step * s.n_var;
#pragma unroll 1
    for (int c = 0; c < ncols; ++c) s.stage[c * R + i] = nodemap_load_value(s.field[c][g], s.scale_factor[c], s.add_offset[c], s.a[c], s.b[c]);
    const int nwork = s.n_step * s.npairs;   // transformData: per forcing step, per pair (externaldata.cpp:1003-1283)
#pragma unroll 1
    for (int q = 0; q < nwork; ++q) {
        const int fstep = q / s.npairs, k = q - fstep * s.npairs;
        double *p0 = s.stage + (size_t)(fstep * s.n_var + s.j0[k]) * R + i, *p1 = s.stage + (size_t)(fstep * s.n_var + s.j1[k]) * R + i;
        if (s.east_west) nf_east_north_point(s.map, s.Re, s.lat[i], s.lon[i], p0, p1);
        if (s.rotate != ROTATE_NONE) {
            const double c = s.rotate == ROTATE_UNIFORM ? s.c : s.cs[i], sn = s.rotate == ROTATE_UNIFORM ? s.s : s.sn[i];
            const double t0 = *p0, t1 = *p1;
            *p0 = c * t0 + sn * t1;      // externaldata.cpp:1255-1256, 1275-1276
            *p1 = -sn * t0 + c * t1;
        }
    }
}

struct ColsArgs {
    const double *stage;            // [n_step*n_var][R]
    int R, N;
    int col[kMaxLoad];              // the staged column of kept column k
    double *out[kMaxLoad];          // [N] each
};

template <int NC>
__global__ void __launch_bounds__(256) k_nodemap_cols_gather(ColsArgs g, const int *__restrict__ v0, const int *__restrict__ v1, const int *__restrict__ v2,
                                                             const double *__restrict__ a0, const double *__restrict__ a1, const double *__restrict__ a2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.N) return;
    const int i0 = v0[i], i1 = v1[i], i2 = v2[i];
    const double w0 = a0[i], w1 = a1[i], w2 = a2[i];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const double *d = g.stage + (size_t)g.col[k] * g.R;
        g.out[k][i] = w0 * d[i0] + w1 * d[i1] + w2 * d[i2];   // InterpFromMeshToMesh2dx.cpp:157-159
    }
}

}  // namespace nodemap
