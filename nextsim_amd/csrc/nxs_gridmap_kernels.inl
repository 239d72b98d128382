// nxs_gridmap_kernels.inl -- the kernels of nxs_gridmap (include/nxs_interp.h): conservative remapping between the mesh and a grid of
// quadrilateral cells with the weights kept on the device as lists.  Textually included by nxs_interp.hip behind the regrid context, whose exact
// locator (locate) and connectivity tables it reads, and behind nxs_remap_core.inl (NXS_HD = __device__), whose per-cell functions it runs with
// NC = 4.  Reference: contrib/bamg/src/ConservativeRemapping.cpp:15-171.  tests/native/gridmap_host.cpp restates the loops around the shared
// functions on the host.
namespace gridmap {

// ConservativeRemapping.cpp:55-61: InterpFromMeshToMesh2dx(elnum, ..., gridX, gridY, true, -1) -- the element holding the P-point, -1 = land
__global__ void __launch_bounds__(256) k_gridmap_seed(InterpDev loc, int G, const double *__restrict__ gx, const double *__restrict__ gy, int *__restrict__ seed) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= G) return;
    const double x = gx[c], y = gy[c];
    int s = -1;
    if (!(x < loc.xmin || x > loc.xmax || y < loc.ymin || y > loc.ymax)) {
        long long dd[3], Bx, By;
        s = locate(loc, x, y, dd, Bx, By);
        if (s >= loc.nels) s = -1;
    }
    seed[c] = s;
}

// one thread per wet cell of the chunk: checkTriangle's walk with lists of kMaxVisitBig entries in global memory.  count = entries, 0 for a failed cell
// (more than kMaxVisitBig triangles, or more than kMaxPoints points in one polygon), which is counted.
__global__ void __launch_bounds__(64) k_gridmap_walk(nxs_remap::OldMesh m, int ncell, const int *__restrict__ cells, const int *__restrict__ seed,
                                                     const double *__restrict__ cornerX, const double *__restrict__ cornerY, int *tris_all, double *w_all,
                                                     nxs_remap::Frame *stack_all, int *__restrict__ count, int *failed) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= ncell) return;
    const int c = cells[i];
    double cx[4], cy[4];
    for (int k = 0; k < 4; ++k) { cx[k] = cornerX[4 * (size_t)c + k]; cy[k] = cornerY[4 * (size_t)c + k]; }
    const int n = nxs_remap::collect_n<4>(m, cx, cy, seed[c], false, tris_all + (size_t)i * nxs_remap::kMaxVisitBig, w_all + (size_t)i * nxs_remap::kMaxVisitBig,
                                          stack_all + (size_t)i * (nxs_remap::kMaxVisitBig + 1), nxs_remap::kMaxVisitBig);
    if (n < 0) atomicAdd(failed, 1);
    count[i] = n < 0 ? 0 : n;
}

// the chunk's lists out of the arena into consecutive entries (off = the exclusive scan of count, off[ncell] = their sum): a wavefront per cell
__global__ void __launch_bounds__(256) k_gridmap_compact(int ncell, const int *__restrict__ off, const int *__restrict__ tris_all, const double *__restrict__ w_all,
                                                         int *__restrict__ tris, double *__restrict__ w) {
    const int i = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (i >= ncell) return;
    const int lo = off[i], n = off[i + 1] - lo;
    for (int k = lane; k < n; k += 64) {
        tris[lo + k] = tris_all[(size_t)i * nxs_remap::kMaxVisitBig + k];
        w[lo + k] = w_all[(size_t)i * nxs_remap::kMaxVisitBig + k];
    }
}

// per row: 1 / area(cell) (ConservativeRemapping.cpp:116-122) and the cell's row number
__global__ void __launch_bounds__(256) k_gridmap_rows(int rows, const int *__restrict__ gridP, const double *__restrict__ cornerX, const double *__restrict__ cornerY,
                                                      double *__restrict__ r_area, int *__restrict__ row_of_cell) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const int c = gridP[i];
    double cx[4], cy[4];
    for (int k = 0; k < 4; ++k) { cx[k] = cornerX[4 * (size_t)c + k]; cy[k] = cornerY[4 * (size_t)c + k]; }
    r_area[i] = nxs_remap::r_cell_area_n<4>(cx, cy);
    row_of_cell[c] = i;
}

// the transposed lists: entries per triangle (integer atomics: the rows are sorted afterwards, so the result does not depend on their order) ...
__global__ void __launch_bounds__(256) k_gridmap_t_count(int n, const int *__restrict__ tris, int *t_count) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) atomicAdd(t_count + tris[e], 1);
}
// ... the index of every entry into its triangle's row, and the cell of every entry (its row by bisection of off)
__global__ void __launch_bounds__(256) k_gridmap_t_fill(int n, int rows, const int *__restrict__ tris, const int *__restrict__ off, const int *__restrict__ gridP,
                                                        const int *__restrict__ t_off, int *cursor, int *__restrict__ t_pos, int *__restrict__ cell) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int t = tris[e];
    t_pos[t_off[t] + atomicAdd(cursor + t, 1)] = e;
    int lo = 0, hi = rows - 1;   // the last row with off[row] <= e (no row is empty)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    cell[e] = gridP[lo];
}

// ConservativeRemappingMeshToGrid (:103-135): one thread per (cell, variable), the variable fastest
__global__ void __launch_bounds__(256) k_gridmap_to_grid(long long total, int nb_var, const int *__restrict__ row_of_cell, const int *__restrict__ off,
                                                         const int *__restrict__ tris, const double *__restrict__ w, const double *__restrict__ r_area,
                                                         const double *__restrict__ in, double miss_val, double *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid / nb_var), var = (int)(gid % nb_var);
    const int row = row_of_cell[c];
    if (row < 0) { out[gid] = miss_val; return; }
    const int lo = off[row];
    out[gid] = nxs_remap::grid_value(in, nb_var, var, tris + lo, w + lo, off[row + 1] - lo, r_area[row]);
}

// The coupler's put (nxs_gridmap_send_rows): GridOutput::updateGridMean's conservative elemental leg with the grid accumulators on the device -- per cell
// ConservativeRemapping.cpp:128-132 and gridoutput.cpp:545: v = 0; v += in[tri*nb_var+var]*w in list order; v *= r_cell_area; data_grid[var][c] += v, and a dry
// cell adds the 0. the reference passes as its missing value there (the += is kept: it turns a -0. of the accumulator into +0.).  One thread per grid cell, all G
// of them; a wet cell walks its list ONCE for the nv <= NV variables col0 .. (k_gridmap_to_grid walks it once per variable and writes [G][nb_var]).  A triangle's
// nb_var accumulators are consecutive doubles; consecutive threads store consecutive entries of each [G] row.  No atomics, no LDS; the NV sums stay in registers
// (builds for 4, 8 and 12; longer lists come in column tiles of 12).  Gather- and latency-bound: the row lengths differ from lane to lane and every entry is a
// dependent load through tris[], so the wavefront runs as long as its longest row -- not bandwidth-bound.
constexpr int kSendTile = 12;
template <int NV>
__global__ void __launch_bounds__(256) k_gridmap_send(int G, int nb_var, int col0, int nv, const int *__restrict__ row_of_cell, const int *__restrict__ off,
                                                      const int *__restrict__ tris, const double *__restrict__ w, const double *__restrict__ r_area,
                                                      const double *__restrict__ in, double *__restrict__ data_grid) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= G) return;
    const int row = row_of_cell[c];
    double v[NV];
    if (row < 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = 0.;
    } else {
        const int lo = off[row];
        nxs_remap::grid_values<NV>(in, nb_var, col0, nv, tris + lo, w + lo, off[row + 1] - lo, r_area[row], v);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (i < nv) data_grid[(size_t)(col0 + i) * G + c] += v[i];
}

// ConservativeRemappingGridToMesh (:138-171) as a gather over the transposed lists: one thread per (triangle, variable)
__global__ void __launch_bounds__(256) k_gridmap_to_mesh(long long total, int nb_var, const int *__restrict__ t_off, const int *__restrict__ t_pos,
                                                         const int *__restrict__ cell, const double *__restrict__ w, const double *__restrict__ in,
                                                         double *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int t = (int)(gid / nb_var), var = (int)(gid % nb_var);
    const int lo = t_off[t];
    out[gid] = nxs_remap::mesh_value(in, nb_var, var, t_pos + lo, t_off[t + 1] - lo, cell, w);
}

// The coupler's receive (nxs_gridmap_receive_rows): up to kMaxReceive element variables, each an [G] field of its own in and an [Ne] row of its own out.
// One thread per triangle: its transposed list is walked ONCE for all variables (k_gridmap_to_mesh walks it once per variable), the transform t * a + b is
// applied as a cell is gathered, factor * x + bias as the row is stored -- consecutive threads store consecutive entries of every row.  Same sums in the same
// order as k_gridmap_to_mesh on the interleaved, transformed input (nxs_remap::receive_values); no atomics.  PERM: cell / w are copies in transposed order.
constexpr int kMaxReceive = 5;
struct ReceiveArgs {
    const double *field[kMaxReceive];
    double *out[kMaxReceive];
    nxs_remap::ReceiveCoef co[kMaxReceive];
};
template <int NV, bool PERM>
__global__ void __launch_bounds__(256) k_gridmap_receive(int nels, const int *__restrict__ t_off, const int *__restrict__ t_pos, const int *__restrict__ cell,
                                                         const double *__restrict__ w, ReceiveArgs r) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nels) return;
    const int lo = t_off[t];
    double v[NV];
    nxs_remap::receive_values<NV>(r.field, r.co, PERM ? nullptr : t_pos, lo, t_off[t + 1] - lo, cell, w, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) r.out[i][t] = v[i];
}
// cell / w in transposed order, for PERM: one thread per entry
__global__ void __launch_bounds__(256) k_gridmap_permute(int n, const int *__restrict__ t_pos, const int *__restrict__ cell, const double *__restrict__ w,
                                                         int *__restrict__ cell_t, double *__restrict__ w_t) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int p = t_pos[k];
    cell_t[k] = cell[p];
    w_t[k] = w[p];
}

}  // namespace gridmap
