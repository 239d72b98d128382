// nxs_nodal_forcing_kernels.inl -- the dynamics' nodal forcing on the device (textually included by nxs_dyn.hip behind the nesting kernels; include/nxs_dyn.h,
// nxs_dyn_forcing_* and nxs_mapx_forward).  externaldata.cpp = model/externaldata.cpp.  The grid data lie [cM][cN][N_data] (row_major == 0) with cN = N + 1 under
// cyclic_x and cM = M + 1 under cyclic_y: the upload leaves the wrap column / row free, the transform kernels walk the M x N points, k_nf_wrap fills the rest.
//   k_mapx_forward   nxs_mapx_forward_point (nxs_mapx_body.inl) on n points: the door of nxs_mapx_forward.
//   k_nf_east_north  transformData's east/north branch for one grid point and one pair (externaldata.cpp:1155-1204): read-modify-write on the two columns of its
//              own point.  gridDim.y picks the pair, so its columns are wave-uniform.
//   k_nf_pole        :1206-1243: one thread per (pair, component) sums the row next to the pole row over x_ind ascending from 0., divides by N and writes the
//              pole row.  Sequential, so the bits are the reference's.
//   k_nf_rotate      :1246-1261: c*a + s*b, -s*a + c*b, every product and sum rounded on its own.
//   k_nf_wrap        interpolateDataset's cyclic copy (:1315-1373): column N = column 0, row M = row 0; the corner cell when both axes are cyclic is the 0. the
//              reference's std::vector holds there (neither of its two loops reaches it).
//   k_nf_ingest      InterpFromGridToMeshx at the nodes (:1436): one thread per node (nxs_grid_to_mesh_body.inl), column j to dst[j][node].
//   k_nf_blend       ExternalData::get for M_wind, M_ocean, M_ssh with coefficients per group (externaldata.cpp:401-403 + 438 LINEAR, the expression of
//              k_blend_forcing; :434 + 438 STEP, which never reads d1).  gridDim.y picks the group.  A lane takes two neighbouring entries with one 16-byte access
//              where the row's start is 16-byte aligned: the u half always, the v half where Nn is even; the v half of an odd Nn and the tail go by scalars
//              (k_nesting_dynamics' rule).
// Plain loads and stores, no LDS, no atomics.  The bodies compile for the host (tests/nodal_forcing_host_kernel.cpp defines the HIP qualifiers away).  The build is
// uncontracted (-ffp-contract=off).

#include "nxs_east_north_body.inl"   // nxs_mapx_body.inl and nf_east_north_point, shared with k_nodemap_source (nxs_nodemap_kernels.inl)

enum { NF_ROWS = 5, NF_SETS = 4, NF_MAX_COLUMNS = 32, NF_MAX_VECTORS = 4, NF_GROUPS = 3 };
static_assert(NF_ROWS == NXS_NF_ROWS && NF_SETS == NXS_NF_SETS && NF_MAX_COLUMNS == NXS_NF_MAX_COLUMNS && NF_MAX_VECTORS == NXS_NF_MAX_VECTORS && NF_GROUPS == NXS_NF_GROUPS,
              "the rows of nxs_dyn_forcing_*");

__global__ void __launch_bounds__(BLOCK) k_mapx_forward(nxs_mapx_polar m, long long n, const double *__restrict__ lat, const double *__restrict__ lon, double *__restrict__ x,
                                                        double *__restrict__ y) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double u, v;
    nxs_mapx_forward_point(m, lat[i], lon[i], &u, &v);
    x[i] = u; y[i] = v;
}

struct NfGrid {                    // the uploaded grid: M x N points in rows of cN cells, N_data columns per cell
    double *data;
    int M, N, cM, cN, N_data;
};
struct NfVectors {
    NfGrid g;
    int npairs;
    int j0[NF_MAX_VECTORS], j1[NF_MAX_VECTORS], east_west[NF_MAX_VECTORS];
    const double *lat, *lon;       // [M], [N] (per_point == 0) or [M*N] each
    int per_point;
    int pole_row, pole_next;       // the row at 90N and the row beside it; -1: no pole row
    nxs_mapx_polar map;
    double R;                      // mapx_Re_km*1000.
    double c, s;                   // cos(-rotation_angle), sin(-rotation_angle)
};

__global__ void __launch_bounds__(BLOCK) k_nf_east_north(NfVectors a) {
    const int k = blockIdx.y;
    if (!a.east_west[k]) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x;   // i = y_ind*N + x_ind
    if (i >= a.g.M * a.g.N) return;
    const int y_ind = i / a.g.N, x_ind = i % a.g.N;
    double *cell = a.g.data + ((size_t)y_ind * a.g.cN + x_ind) * a.g.N_data;
    const double lat = a.per_point ? a.lat[i] : a.lat[y_ind], lon = a.per_point ? a.lon[i] : a.lon[x_ind];
    nf_east_north_point(a.map, a.R, lat, lon, cell + a.j0[k], cell + a.j1[k]);
}

__global__ void __launch_bounds__(BLOCK) k_nf_pole(NfVectors a) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;   // (pair, component)
    if (t >= 2 * a.npairs) return;
    const int k = t >> 1;
    if (!a.east_west[k] || a.pole_row < 0) return;
    const int j = (t & 1) ? a.j1[k] : a.j0[k];
    const size_t ND = (size_t)a.g.N_data;
    double tmp = 0.;
    for (int x_ind = 0; x_ind < a.g.N; ++x_ind) tmp = tmp + a.g.data[((size_t)a.pole_next * a.g.cN + x_ind) * ND + j];
    tmp = tmp / a.g.N;
    for (int x_ind = 0; x_ind < a.g.N; ++x_ind) a.g.data[((size_t)a.pole_row * a.g.cN + x_ind) * ND + j] = tmp;
}

__global__ void __launch_bounds__(BLOCK) k_nf_rotate(NfVectors a) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.g.M * a.g.N) return;
    const int y_ind = i / a.g.N, x_ind = i % a.g.N;
    double *cell = a.g.data + ((size_t)y_ind * a.g.cN + x_ind) * a.g.N_data;
    const double east = cell[a.j0[k]], north = cell[a.j1[k]];
    cell[a.j0[k]] = a.c * east + a.s * north;
    cell[a.j1[k]] = -a.s * east + a.c * north;
}

__global__ void __launch_bounds__(BLOCK) k_nf_wrap(NfGrid g) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int ncol = g.cN != g.N ? g.M : 0, nrow = g.cM != g.M ? g.N : 0, corner = (g.cN != g.N && g.cM != g.M) ? 1 : 0;
    const size_t ND = (size_t)g.N_data;
    if (t < ncol) {                      // cell (t, N) = cell (t, 0)
        const double *src = g.data + ((size_t)t * g.cN) * ND;
        double *dst = g.data + ((size_t)t * g.cN + g.N) * ND;
        for (int j = 0; j < g.N_data; ++j) dst[j] = src[j];
    } else if (t < ncol + nrow) {        // cell (M, x) = cell (0, x)
        const int x_ind = t - ncol;
        const double *src = g.data + (size_t)x_ind * ND;
        double *dst = g.data + ((size_t)g.M * g.cN + x_ind) * ND;
        for (int j = 0; j < g.N_data; ++j) dst[j] = src[j];
    } else if (t < ncol + nrow + corner) {
        double *dst = g.data + ((size_t)g.M * g.cN + g.N) * ND;
        for (int j = 0; j < g.N_data; ++j) dst[j] = 0.;
    }
}

struct NfIngest {
    G2M g;                        // g.nods = Nn, g.M / g.N = cM / cN, g.N_data = the columns of data
    const double *rx, *ry;        // [Nn] the targets of the dataset
    double *dst[NF_MAX_COLUMNS];  // column j -> its [Nn] half-row of a snapshot; NULL: skipped
};
struct NfColumns {
    double *const *dst;
    int i;
    __device__ __forceinline__ bool wants(int j) const { return dst[j] != nullptr; }
    __device__ __forceinline__ void put(int j, double v) const { dst[j][i] = v; }
};

__global__ void __launch_bounds__(BLOCK) k_nf_ingest(NfIngest a, const double *__restrict__ data) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.g.nods) return;
    grid_to_mesh_point(a.g, data, a.rx[i], a.ry[i], NfColumns{a.dst, i});
}

struct alignas(16) NfPair { double a, b; };
struct NfGroup {
    const double *d0, *d1;   // the snapshots (d1 is not read under NXS_TF_STEP)
    double *out;             // M_wind / M_ocean [2*Nn], M_ssh [Nn]
    int halves;              // 2: [u | v]; 1: ssh
    double c0, c1, factor, bias;
    int mode;                // NXS_TF_LINEAR or NXS_TF_STEP (an OFF group is not in the table)
};
struct NfBlend {
    int Nn, ngroups;
    NfGroup grp[NF_GROUPS];  // packed: gridDim.y = ngroups
};

__device__ __forceinline__ double nf_value(const NfGroup &r, double d0, double d1) {
    return r.mode == NXS_TF_LINEAR ? r.factor * (r.c0 * d0 + r.c1 * d1) + r.bias : r.factor * d0 + r.bias;
}
__device__ __forceinline__ void nf_blend_one(const NfGroup &r, size_t i) { r.out[i] = nf_value(r, r.d0[i], r.mode == NXS_TF_LINEAR ? r.d1[i] : 0.); }
__device__ __forceinline__ void nf_blend_pair(const NfGroup &r, size_t i) {
    const NfPair p0 = *reinterpret_cast<const NfPair *>(r.d0 + i);
    NfPair p1{0., 0.};
    if (r.mode == NXS_TF_LINEAR) p1 = *reinterpret_cast<const NfPair *>(r.d1 + i);
    *reinterpret_cast<NfPair *>(r.out + i) = NfPair{nf_value(r, p0.a, p1.a), nf_value(r, p0.b, p1.b)};
}

__global__ void __launch_bounds__(BLOCK) k_nf_blend(NfBlend b) {
    const NfGroup &r = b.grp[blockIdx.y];
    const int i = 2 * (blockIdx.x * BLOCK + threadIdx.x);   // this lane's first node
    const size_t Nn = (size_t)b.Nn;
    if (i + 1 < b.Nn) {
        nf_blend_pair(r, i);
        if (r.halves == 2) {
            if ((b.Nn & 1) == 0) nf_blend_pair(r, Nn + i);
            else { nf_blend_one(r, Nn + i); nf_blend_one(r, Nn + i + 1); }   // (v + i is 8 bytes off a 16-byte boundary)
        }
    } else if (i < b.Nn) {   // odd Nn: the last node alone
        nf_blend_one(r, i);
        if (r.halves == 2) nf_blend_one(r, Nn + i);
    }
}
