// nxs_thermo_forcing_kernels.inl -- thermo()'s element forcing on the device (textually included by nxs_dyn.hip behind the slab kernels; include/nxs_dyn.h,
// nxs_dyn_thermo_forcing_*).  externaldata.cpp = model/externaldata.cpp.
//   k_thermo_forcing_blend    ExternalData::get for the ten [Ne] rows of nxs_dyn_flux_atmosphere / nxs_dyn_column_forcing (externaldata.cpp:401-403, 434, 438): up to
//              twenty snapshot rows in, ten rows out.  gridDim.y picks the row, so its mode, coefficients and pointers are wave-uniform (scalar loads from the
//              kernel arguments) and the branch on the mode does not diverge.  A lane takes two neighbouring elements with one 16-byte access per row (every row is
//              an allocation of its own, so it is 16-byte aligned); the last element of an odd Ne is a scalar tail.  Plain stores: the next launch reads the rows.
//              A STEP row never touches d1.  No LDS, no atomics.
//   k_thermo_forcing_ingest   InterpFromGridToMeshx at the element barycentres (externaldata.cpp:1436): one thread per element finds the grid interval once
//              (nxs_grid_to_mesh_body.inl, the arithmetic of k_grid_to_mesh) and loops over the columns; column j goes to dst[j][e], one contiguous [Ne] stream per
//              column -- no interleaved scratch.  A column without a destination is never read.
// Both bodies compile for the host (tests/thermo_forcing_host_kernel.cpp defines the HIP qualifiers away).  The build is uncontracted (-ffp-contract=off): a*b + c is
// two roundings, and the association is the reference's.

#include "nxs_grid_to_mesh_body.inl"

enum { TF_ROWS = 10, TF_SETS = 4, TF_MAX_COLUMNS = 32 };
static_assert(TF_ROWS == NXS_TF_ROWS && TF_SETS == NXS_TF_SETS && TF_MAX_COLUMNS == NXS_TF_MAX_COLUMNS, "the rows of nxs_dyn_thermo_forcing_*");

struct alignas(16) TfPair { double a, b; };   // two neighbouring elements of a row: one 16-byte access

struct TfRow {
    const double *d0, *d1;   // the snapshots (d1 is not read under NXS_TF_STEP: it may be NULL)
    double *out;             // d_flux_atm[k] / d_col_forcing[k - 5]
    double c0, c1, factor, bias;
    int mode;                // NXS_TF_LINEAR or NXS_TF_STEP (an OFF row is not in the table)
};
struct TfBlend {
    int Ne, nrows;
    TfRow row[TF_ROWS];      // the rows to write, packed: gridDim.y = nrows
};

// ExternalData::get for one element: externaldata.cpp:401-403 + 438 (LINEAR), :434 + 438 (STEP)
__device__ __forceinline__ double tf_linear(const TfRow &r, double d0, double d1) { return r.factor * (r.c0 * d0 + r.c1 * d1) + r.bias; }
__device__ __forceinline__ double tf_step(const TfRow &r, double d0) { return r.factor * d0 + r.bias; }

__global__ void __launch_bounds__(BLOCK) k_thermo_forcing_blend(TfBlend b) {
    const TfRow &r = b.row[blockIdx.y];
    const int i = 2 * (blockIdx.x * BLOCK + threadIdx.x);   // this lane's first element
    if (i + 1 < b.Ne) {
        const TfPair p0 = *reinterpret_cast<const TfPair *>(r.d0 + i);
        TfPair o;
        if (r.mode == NXS_TF_LINEAR) {
            const TfPair p1 = *reinterpret_cast<const TfPair *>(r.d1 + i);
            o.a = tf_linear(r, p0.a, p1.a);
            o.b = tf_linear(r, p0.b, p1.b);
        } else {
            o.a = tf_step(r, p0.a);
            o.b = tf_step(r, p0.b);
        }
        *reinterpret_cast<TfPair *>(r.out + i) = o;
    } else if (i < b.Ne) {   // odd Ne: the last element alone
        r.out[i] = r.mode == NXS_TF_LINEAR ? tf_linear(r, r.d0[i], r.d1[i]) : tf_step(r, r.d0[i]);
    }
}

struct TfIngest {
    G2M g;                        // g.nods = Ne, g.N_data = the columns of data
    const double *rx, *ry;        // [Ne] the targets of the dataset
    double *dst[TF_MAX_COLUMNS];  // column j -> its [Ne] snapshot row; NULL: skipped
};
struct TfColumns {                // where grid_to_mesh_point puts element e's columns
    double *const *dst;
    int e;
    __device__ __forceinline__ bool wants(int j) const { return dst[j] != nullptr; }
    __device__ __forceinline__ void put(int j, double v) const { dst[j][e] = v; }
};

__global__ void __launch_bounds__(BLOCK) k_thermo_forcing_ingest(TfIngest a, const double *__restrict__ data) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= a.g.nods) return;
    grid_to_mesh_point(a.g, data, a.rx[e], a.ry[e], TfColumns{a.dst, e});
}
