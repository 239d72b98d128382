// nxs_drifters.inl -- the drifters on the device (textually included by nxs_interp.hip, behind InterpDev / locate() / regrid_tables; interface:
// nxs_drifters.hpp).
//
// Reference: FiniteElement::checkMoveDrifters (FE.cpp:8375-8397), checkUpdateDrifters (FE.cpp:8403-8437), Drifters::move (model/drifters.cpp:468-506),
// Drifters::updateConc (drifters.cpp:512-542), Drifters::maskXY (drifters.cpp:548-579).  Both interpolations are InterpFromMeshToMesh2dx with
// isdefault = true and default 0.: a drifter outside the mesh's bounding box (InterpFromMeshToMesh2dx.cpp:92) or in no triangle of the mesh gets 0.
// Inside the mesh the integer plane, the determinants and the operand order are k_interp's, so the bits are bamg's.
//
// What differs from Locator::build: the coordinates never leave the device.  The bounding box is a two-stage min/max reduction, the host derives
// SetIntCoor's pmin / coefIcoor from those four doubles (Mesh.cpp:3441-3468), a kernel truncates the coordinates into the plane, and the bucket
// grid is built by the kernels of nxs_regrid_tables.inl over the handle's own triangle arrays.  No convex completion and no boundary edges:
// isdefault is true on both calls.

namespace nxs_drifters {
namespace {

constexpr int BBOX_BLOCKS = 512;

// stage 1: per-block partial [xmin, xmax, ymin, ymax, #NaN] of x0 (+ UM); comparisons as std::min / std::max make them (a NaN never wins: it is counted)
__global__ void __launch_bounds__(256) k_bbox_partial(int n, const double *__restrict__ x0, const double *__restrict__ y0, const double *__restrict__ UM,
                                                      double *__restrict__ part) {
    __shared__ double sh[5][256];
    double v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        double x = x0[i], y = y0[i];
        if (UM) { x += UM[i]; y += UM[(size_t)n + i]; }
        if (x != x || y != y) v[4] += 1.;
        if (x < v[0]) v[0] = x;
        if (x > v[1]) v[1] = x;
        if (y < v[2]) v[2] = y;
        if (y > v[3]) v[3] = y;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < (unsigned)off) {
            const int o = threadIdx.x + off;
            if (sh[0][o] < sh[0][threadIdx.x]) sh[0][threadIdx.x] = sh[0][o];
            if (sh[1][o] > sh[1][threadIdx.x]) sh[1][threadIdx.x] = sh[1][o];
            if (sh[2][o] < sh[2][threadIdx.x]) sh[2][threadIdx.x] = sh[2][o];
            if (sh[3][o] > sh[3][threadIdx.x]) sh[3][threadIdx.x] = sh[3][o];
            sh[4][threadIdx.x] += sh[4][o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 5) part[(size_t)blockIdx.x * 5 + threadIdx.x] = sh[threadIdx.x][0];
}
// stage 2: one workgroup over the partials
__global__ void __launch_bounds__(256) k_bbox_final(int nparts, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double sh[5][256];
    double v[5] = {INFINITY, -INFINITY, INFINITY, -INFINITY, 0.};
    for (int b = threadIdx.x; b < nparts; b += 256) {
        const double *p = part + (size_t)b * 5;
        if (p[0] < v[0]) v[0] = p[0];
        if (p[1] > v[1]) v[1] = p[1];
        if (p[2] < v[2]) v[2] = p[2];
        if (p[3] > v[3]) v[3] = p[3];
        v[4] += p[4];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < (unsigned)off) {
            const int o = threadIdx.x + off;
            if (sh[0][o] < sh[0][threadIdx.x]) sh[0][threadIdx.x] = sh[0][o];
            if (sh[1][o] > sh[1][threadIdx.x]) sh[1][threadIdx.x] = sh[1][o];
            if (sh[2][o] < sh[2][threadIdx.x]) sh[2][threadIdx.x] = sh[2][o];
            if (sh[3][o] > sh[3][threadIdx.x]) sh[3][threadIdx.x] = sh[3][o];
            sh[4][threadIdx.x] += sh[4][o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 5) out[threadIdx.x] = sh[threadIdx.x][0];
}

// R2ToI2 of every vertex (Mesh.cpp:3688-3690), with the range check of nxs_hull::int_plane; *bad counts the vertices that fail it
__global__ void __launch_bounds__(256) k_int_plane(int n, const double *__restrict__ x0, const double *__restrict__ y0, const double *__restrict__ UM, double coef,
                                                   double pminx, double pminy, int *__restrict__ ix, int *__restrict__ iy, int *bad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double x = x0[i], y = y0[i];
    if (UM) { x += UM[i]; y += UM[(size_t)n + i]; }
    const double fx = coef * (x - pminx), fy = coef * (y - pminy);
    if (!(fx >= 0. && fx < 1073741824. && fy >= 0. && fy < 1073741824.)) { atomicAdd(bad, 1); ix[i] = 0; iy[i] = 0; return; }
    ix[i] = (int)fx; iy[i] = (int)fy;
}

// Drifters::move for one set: M_UT interpolated at the drifters (P1, the operand order of InterpFromMeshToMesh2dx.cpp:151-156), x += du, y += dv.
// UT is the handle's [u | v] vector: the reference's interleaving copy (drifters.cpp:483-487) moves values and changes none.
// found: 0 = in no triangle, 1 = in an owned element, 2 = in a ghost element (left where it is: the rank that owns the element moves it)
__global__ void __launch_bounds__(256) k_drifters_move(InterpDev d, int n, int Neo, const double *__restrict__ UT, double *__restrict__ x, double *__restrict__ y,
                                                       int *__restrict__ found) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = x[i], py = y[i];
    int f = 0;
    if (!(px < d.xmin || px > d.xmax || py < d.ymin || py > d.ymax)) {
        long long dd[3] = {0, 0, 0}, Bx, By;
        const int it = locate(d, px, py, dd, Bx, By);
        if (it >= 0) {
            f = it < Neo ? 1 : 2;
            if (f == 1) {
                const long long det = dd[0] + dd[1] + dd[2];
                const double a0 = (double)dd[0] / det, a1 = (double)dd[1] / det, a2 = (double)dd[2] / det;
                const int i0 = d.t0[it], i1 = d.t1[it], i2 = d.t2[it];
                const double *V = UT + d.nods;
                const double du = a0 * UT[i0] + a1 * UT[i1] + a2 * UT[i2];
                const double dv = a0 * V[i0] + a1 * V[i1] + a2 * V[i2];
                x[i] = px + du;
                y[i] = py + dv;
            }
        }
    }
    found[i] = f;
}

// Drifters::updateConc for one set: P0 look-up in the displaced mesh, then std::max(0., std::min(1., v)) as the two comparisons the standard
// library makes (a NaN gives 1)
__global__ void __launch_bounds__(256) k_drifters_conc(InterpDev d, int n, int Neo, const double *__restrict__ conc_el, const double *__restrict__ x,
                                                       const double *__restrict__ y, double *__restrict__ conc, int *__restrict__ found) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = x[i], py = y[i];
    int f = 0;
    double v = 0.;
    if (!(px < d.xmin || px > d.xmax || py < d.ymin || py > d.ymax)) {
        long long dd[3] = {0, 0, 0}, Bx, By;
        const int it = locate(d, px, py, dd, Bx, By);
        if (it >= 0) { f = it < Neo ? 1 : 2; v = conc_el[it]; }
    }
    const double lo = (v < 1.) ? v : 1.;     // std::min(1., v)
    conc[i] = (0. < lo) ? lo : 0.;           // std::max(0., lo)
    found[i] = f;
}

// maskXY's test: flag[i] = conc[i] > conc_lim && id[i] among the (sorted) keepers; nk < 0: every id is kept.  flag[n] = 0 (the scan leaves the count there)
__global__ void __launch_bounds__(256) k_drifters_flags(int n, const double *__restrict__ conc, const int *__restrict__ id, double conc_lim,
                                                        const int *__restrict__ keepers, int nk, int *__restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { flag[n] = 0; return; }
    bool keep = conc[i] > conc_lim;
    if (keep && nk >= 0) {
        const int want = id[i];
        int lo = 0, hi = nk;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (keepers[mid] < want) lo = mid + 1; else hi = mid; }
        keep = lo < nk && keepers[lo] == want;
    }
    flag[i] = keep ? 1 : 0;
}
// the survivors in their order: pos = the exclusive scan of the flags
__global__ void __launch_bounds__(256) k_drifters_scatter(int n, const int *__restrict__ pos, const double *__restrict__ x, const double *__restrict__ y,
                                                          const int *__restrict__ id, const double *__restrict__ conc, const int *__restrict__ found,
                                                          double *__restrict__ x2, double *__restrict__ y2, int *__restrict__ id2, double *__restrict__ conc2,
                                                          int *__restrict__ found2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = pos[i];
    if (pos[i + 1] == p) return;
    x2[p] = x[i]; y2[p] = y[i]; id2[p] = id[i]; conc2[p] = conc[i]; found2[p] = found[i];
}

struct Set {
    bool exists = false;
    int n = 0, cap = -1, cur = 0;
    DevBuf<double> x[2], y[2], conc[2];
    DevBuf<int> id[2], found[2], flag;
};

struct DevLocator {
    InterpDev d{};
    DevBuf<int> ix, iy, off, cursor, wide, nwide, bad, tri;
    size_t tri_cap = 0;
    bool sized = false, valid = false;
    double bbox[4] = {0, 0, 0, 0};
    void drop() {   // set_mesh: the sizes change
        for (DevBuf<int> *b : {&ix, &iy, &off, &cursor, &wide, &nwide, &bad, &tri})
            if (b->p) { (void)hipFree(b->p); b->p = nullptr; }
        tri_cap = 0; sized = valid = false;
    }
};

inline int grid_blocks(long long n) { return (int)((n + 255) / 256); }

}  // namespace

struct State {
    Set sets[NXS_DRIFTER_SETS];
    DevLocator loc[2];                 // [0] the undisplaced mesh, [1] the mesh displaced by M_UM
    DevBuf<double> part, box;          // partials of the bounding-box reduction, its result
    bool own_box_valid[2] = {false, false};
    double own_box[2][4] = {};
    bool timing = false, timed = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[5] = {0, 0, 0, 0, 0};    // [4] the launch of nxs_means_points_kernels.inl
    double mp_ms[2] = {0, 0};          // the last nxs_dyn_means_points_update: its locator build (0: none was needed), its kernel
    unsigned builds = 0;               // locator builds so far
};

namespace {

#define DCHK(call)                                                                                                       \
    do {                                                                                                                 \
        hipError_t _e = (call);                                                                                          \
        if (_e != hipSuccess) { err = std::string(#call " failed: ") + hipGetErrorString(_e); return NXS_ERR_HIP; }       \
    } while (0)

struct Timed {   // events around a group of launches when the handle's option "drifters_timing" is set
    State *s; hipStream_t st; int slot;
    Timed(State *s_, hipStream_t st_, int slot_) : s(s_), st(st_), slot(slot_) {
        if (!s->timing) return;
        for (auto &e : s->ev) if (!e) (void)hipEventCreate(&e);
        (void)hipEventRecord(s->ev[0], st);
    }
    ~Timed() {
        if (!s->timing) return;
        (void)hipEventRecord(s->ev[1], st);
        float t = 0.f;
        if (hipEventSynchronize(s->ev[1]) == hipSuccess && hipEventElapsedTime(&t, s->ev[0], s->ev[1]) == hipSuccess) { s->ms[slot] = t; s->timed = true; }
    }
};

int own_bbox(State *s, hipStream_t st, const MeshView &m, const double *UM, double out[4], std::string &err) {
    const int which = UM ? 1 : 0;
    if (!s->own_box_valid[which]) {
        if (!s->part.p && (s->part.alloc((size_t)BBOX_BLOCKS * 5) || s->box.alloc(5))) { err = "device allocation failed"; return NXS_ERR_HIP; }
        const int nb = std::min(BBOX_BLOCKS, grid_blocks(m.Nn));
        hipLaunchKernelGGL(k_bbox_partial, dim3(nb), dim3(256), 0, st, m.Nn, m.x0, m.y0, UM, s->part.p);
        hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(256), 0, st, nb, (const double *)s->part.p, s->box.p);
        double r[5];
        DCHK(hipMemcpyAsync(r, s->box.p, sizeof r, hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
        if (r[4] != 0.) { err = "a coordinate of the mesh is NaN"; return NXS_ERR_INVALID; }
        for (int k = 0; k < 4; ++k) s->own_box[which][k] = r[k];
        s->own_box_valid[which] = true;
    }
    for (int k = 0; k < 4; ++k) out[k] = s->own_box[which][k];
    return NXS_OK;
}

// The sibling of Locator::build for coordinates that are on the device: integer plane of `box` (xmin, xmax, ymin, ymax: this mesh's own, or the box of
// the global mesh a rank's partition belongs to), bucket grid over the handle's triangle arrays.
int build_locator(State *s, hipStream_t st, const MeshView &m, const double *UM, const double box[4], std::string &err) {
    DevLocator &L = s->loc[UM ? 1 : 0];
    Timed tm(s, st, 0);
    L.valid = false;
    // ---- SetIntCoor (Mesh.cpp:3441-3468), as nxs_hull::int_plane
    double pminx = box[0], pmaxx = box[1], pminy = box[2], pmaxy = box[3];
    const double DDx = (pmaxx - pminx) * 0.05, DDy = (pmaxy - pminy) * 0.05;
    pminx = pminx - DDx; pminy = pminy - DDy;
    pmaxx = pmaxx + DDx; pmaxy = pmaxy + DDy;
    const double coef = 1073741823. / std::max(pmaxx - pminx, pmaxy - pminy);
    if (!(coef > 0.) || !(coef < 1e300)) { err = "coefIcoor should be positive, a problem in the geometry is likely"; return NXS_ERR_INVALID; }
    int G = 1;
    while ((long long)G * G * 2 < m.Ne && G < 4096) G <<= 1;
    int shift = 30;
    for (int g = G; g > 1; g >>= 1) --shift;
    const size_t ncell = (size_t)G * G;
    if (!L.sized) {
        if (L.ix.alloc(m.Nn) || L.iy.alloc(m.Nn) || L.off.alloc(ncell + 1) || L.cursor.alloc(ncell) || L.wide.alloc(m.Ne) || L.nwide.alloc(1) || L.bad.alloc(1)) {
            err = "device allocation failed"; return NXS_ERR_HIP;
        }
        L.sized = true;
    }
    DCHK(hipMemsetAsync(L.bad.p, 0, sizeof(int), st));
    DCHK(hipMemsetAsync(L.off.p, 0, (ncell + 1) * sizeof(int), st));
    DCHK(hipMemsetAsync(L.cursor.p, 0, ncell * sizeof(int), st));
    DCHK(hipMemsetAsync(L.nwide.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_int_plane, dim3(grid_blocks(m.Nn)), dim3(256), 0, st, m.Nn, m.x0, m.y0, UM, coef, pminx, pminy, L.ix.p, L.iy.p, L.bad.p);
    // ---- bucket grid: count -> scan -> fill -> sort every cell's list ascending (nxs_regrid_tables.inl)
    hipLaunchKernelGGL(regrid_tables::k_grid_count, dim3(grid_blocks(m.Ne)), dim3(256), 0, st, m.Ne, m.t0, m.t1, m.t2, (const int *)L.ix.p, (const int *)L.iy.p, shift, G,
                       L.off.p, L.wide.p, L.nwide.p);
    int two[2] = {0, 0};
    DCHK(hipMemcpyAsync(&two[0], L.bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    DCHK(hipMemcpyAsync(&two[1], L.nwide.p, sizeof(int), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    if (two[0] > 0) {
        err = "a coordinate of the mesh is NaN or outside the bounding box given (" + std::to_string(two[0]) + " nodes)";
        return NXS_ERR_INVALID;
    }
    const int n_wide = two[1];
    if (n_wide > 0)
        hipLaunchKernelGGL(regrid_tables::k_grid_count_wide, dim3(n_wide), dim3(256), 0, st, (const int *)L.wide.p, m.t0, m.t1, m.t2, (const int *)L.ix.p, (const int *)L.iy.p,
                           shift, G, L.off.p);
    DCHK(regrid_tables::exclusive_scan(L.off.p, (int)(ncell + 1), st));
    int total = 0;
    DCHK(hipMemcpyAsync(&total, L.off.p + ncell, sizeof(int), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    if ((size_t)total > L.tri_cap || !L.tri.p) {
        const size_t cap = (size_t)total + (size_t)total / 4 + 16;
        if (L.tri.alloc(cap)) { err = "device allocation failed"; return NXS_ERR_HIP; }
        L.tri_cap = cap;
    }
    hipLaunchKernelGGL(regrid_tables::k_grid_fill, dim3(grid_blocks(m.Ne)), dim3(256), 0, st, m.Ne, m.t0, m.t1, m.t2, (const int *)L.ix.p, (const int *)L.iy.p, shift, G,
                       (const int *)L.off.p, L.cursor.p, L.tri.p);
    if (n_wide > 0)
        hipLaunchKernelGGL(regrid_tables::k_grid_fill_wide, dim3(n_wide), dim3(256), 0, st, (const int *)L.wide.p, m.t0, m.t1, m.t2, (const int *)L.ix.p, (const int *)L.iy.p,
                           shift, G, (const int *)L.off.p, L.cursor.p, L.tri.p);
    hipLaunchKernelGGL(regrid_tables::k_rows_sort, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, st, (int)ncell, (const int *)L.off.p, L.tri.p, 0);
    DCHK(hipGetLastError());
    InterpDev &d = L.d;
    d = InterpDev{};
    d.nods = m.Nn; d.nels = m.Ne; d.nels_all = m.Ne; d.N_data = 1; d.nodal = 1;
    d.t0 = m.t0; d.t1 = m.t1; d.t2 = m.t2; d.ix = L.ix.p; d.iy = L.iy.p;
    d.G = G; d.shift = shift; d.cell_off = L.off.p; d.cell_tri = L.tri.p;
    d.coef = coef; d.pminx = pminx; d.pminy = pminy;
    d.xmin = box[0]; d.xmax = box[1]; d.ymin = box[2]; d.ymax = box[3];
    d.isdefault = 1; d.defaultvalue = 0.;
    for (int k = 0; k < 4; ++k) L.bbox[k] = box[k];
    L.valid = true;
    ++s->builds;
    return NXS_OK;
}

int ensure_locator(State *s, hipStream_t st, const MeshView &m, const double *UM, const double *bbox, std::string &err) {
    double box[4];
    if (bbox) {
        for (int k = 0; k < 4; ++k) box[k] = bbox[k];
        if (!(box[0] <= box[1]) || !(box[2] <= box[3])) { err = "bbox must be xmin, xmax, ymin, ymax"; return NXS_ERR_INVALID; }
    } else if (int rc = own_bbox(s, st, m, UM, box, err)) return rc;
    DevLocator &L = s->loc[UM ? 1 : 0];
    if (L.valid && std::memcmp(L.bbox, box, sizeof box) == 0) return NXS_OK;
    return build_locator(s, st, m, UM, box, err);
}

int check_set(int set, std::string &err) {
    if (set < 0 || set >= NXS_DRIFTER_SETS) { err = "drifter set " + std::to_string(set) + " out of range (0.." + std::to_string(NXS_DRIFTER_SETS - 1) + ")"; return NXS_ERR_INVALID; }
    return NXS_OK;
}
int existing_set(State *s, int set, std::string &err) {
    if (int rc = check_set(set, err)) return rc;
    if (!s->sets[set].exists) { err = "drifter set " + std::to_string(set) + " does not exist (nxs_dyn_drifters_set)"; return NXS_ERR_STATE; }
    return NXS_OK;
}

}  // namespace

State *create() { return new State(); }
void destroy(State *s) {
    if (!s) return;
    for (auto &e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;
}
void mesh_changed(State *s) {
    for (auto &L : s->loc) L.drop();
    s->own_box_valid[0] = s->own_box_valid[1] = false;
}
void state_changed(State *s) { s->loc[1].valid = false; s->own_box_valid[1] = false; }
void set_timing(State *s, bool on) { s->timing = on; s->timed = false; }
bool timing(const State *s, double ms[4]) {
    for (int k = 0; k < 4; ++k) ms[k] = s->ms[k];
    return s->timed;
}
bool any_set(const State *s) {
    for (const auto &q : s->sets) if (q.exists) return true;
    return false;
}
bool has_set(const State *s, int set) { return set >= 0 && set < NXS_DRIFTER_SETS && s->sets[set].exists; }

int set(State *s, hipStream_t st, int set, int32_t n, const double *x, const double *y, const int32_t *id, std::string &err) {
    if (int rc = check_set(set, err)) return rc;
    if (n < 0 || (n > 0 && (!x || !y || !id))) { err = "drifters_set: n < 0 or a NULL array"; return NXS_ERR_INVALID; }
    Set &q = s->sets[set];
    if (n > q.cap) {
        for (int b = 0; b < 2; ++b)
            if (q.x[b].alloc(n) || q.y[b].alloc(n) || q.conc[b].alloc(n) || q.id[b].alloc(n) || q.found[b].alloc(n)) { q.cap = -1; q.exists = false; err = "device allocation failed"; return NXS_ERR_HIP; }
        if (q.flag.alloc((size_t)n + 1)) { q.cap = -1; q.exists = false; err = "device allocation failed"; return NXS_ERR_HIP; }
        q.cap = n;
    }
    q.cur = 0; q.n = n; q.exists = true;
    if (n > 0) {
        DCHK(hipMemcpyAsync(q.x[0].p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        DCHK(hipMemcpyAsync(q.y[0].p, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        DCHK(hipMemcpyAsync(q.id[0].p, id, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
        DCHK(hipMemsetAsync(q.conc[0].p, 0, (size_t)n * sizeof(double), st));
        DCHK(hipMemsetAsync(q.found[0].p, 0, (size_t)n * sizeof(int), st));
        DCHK(hipStreamSynchronize(st));   // the caller's arrays may go away
    }
    return NXS_OK;
}

int clear(State *s, int set) {
    std::string err;
    if (int rc = check_set(set, err)) return rc;
    s->sets[set].exists = false; s->sets[set].n = 0;   // (the buffers are kept for the next nxs_dyn_drifters_set)
    return NXS_OK;
}

int mesh_bbox(State *s, hipStream_t st, const MeshView &m, const double *UM, double out[4], std::string &err) { return own_bbox(s, st, m, UM, out, err); }

int move(State *s, hipStream_t st, const MeshView &m, const double *UT, const double *bbox, std::string &err) {
    bool work = false;
    for (const auto &q : s->sets) work = work || (q.exists && q.n > 0);
    if (!work) return NXS_OK;
    if (int rc = ensure_locator(s, st, m, nullptr, bbox, err)) return rc;
    Timed tm(s, st, 1);
    for (auto &q : s->sets)
        if (q.exists && q.n > 0)
            hipLaunchKernelGGL(k_drifters_move, dim3(grid_blocks(q.n)), dim3(256), 0, st, s->loc[0].d, q.n, m.Neo, UT, q.x[q.cur].p, q.y[q.cur].p, q.found[q.cur].p);
    DCHK(hipGetLastError());
    return NXS_OK;
}

int conc(State *s, hipStream_t st, const MeshView &m, const double *UM, const double *conc_el, int set, const double *bbox, double *conc_host, std::string &err) {
    if (int rc = existing_set(s, set, err)) return rc;
    Set &q = s->sets[set];
    if (q.n == 0) return NXS_OK;
    if (int rc = ensure_locator(s, st, m, UM, bbox, err)) return rc;
    {
        Timed tm(s, st, 2);
        hipLaunchKernelGGL(k_drifters_conc, dim3(grid_blocks(q.n)), dim3(256), 0, st, s->loc[1].d, q.n, m.Neo, conc_el, (const double *)q.x[q.cur].p, (const double *)q.y[q.cur].p,
                           q.conc[q.cur].p, q.found[q.cur].p);
        DCHK(hipGetLastError());
    }
    if (conc_host) {
        DCHK(hipMemcpyAsync(conc_host, q.conc[q.cur].p, (size_t)q.n * sizeof(double), hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
    }
    return NXS_OK;
}

int mask(State *s, hipStream_t st, int set, double conc_lim, const int32_t *keepers, int32_t n_keepers, int32_t *n_left, std::string &err) {
    if (int rc = existing_set(s, set, err)) return rc;
    if (keepers && n_keepers < 0) { err = "drifters_mask: n_keepers < 0"; return NXS_ERR_INVALID; }
    Set &q = s->sets[set];
    if (q.n == 0) { if (n_left) *n_left = 0; return NXS_OK; }   // drifters.cpp:553-554
    DevBuf<int> dk;
    int nk = -1;
    if (keepers) {
        std::vector<int> k(keepers, keepers + n_keepers);
        std::sort(k.begin(), k.end());
        nk = n_keepers;
        if (dk.alloc(k.size())) { err = "device allocation failed"; return NXS_ERR_HIP; }
        if (nk > 0) DCHK(hipMemcpyAsync(dk.p, k.data(), k.size() * sizeof(int), hipMemcpyHostToDevice, st));
        DCHK(hipStreamSynchronize(st));
    }
    const int a = q.cur, b = 1 - q.cur;
    int left = 0;
    {
        Timed tm(s, st, 3);
        hipLaunchKernelGGL(k_drifters_flags, dim3(grid_blocks((long long)q.n + 1)), dim3(256), 0, st, q.n, (const double *)q.conc[a].p, (const int *)q.id[a].p, conc_lim,
                           (const int *)dk.p, nk, q.flag.p);
        DCHK(regrid_tables::exclusive_scan(q.flag.p, q.n + 1, st));
        hipLaunchKernelGGL(k_drifters_scatter, dim3(grid_blocks(q.n)), dim3(256), 0, st, q.n, (const int *)q.flag.p, (const double *)q.x[a].p, (const double *)q.y[a].p,
                           (const int *)q.id[a].p, (const double *)q.conc[a].p, (const int *)q.found[a].p, q.x[b].p, q.y[b].p, q.id[b].p, q.conc[b].p, q.found[b].p);
        DCHK(hipMemcpyAsync(&left, q.flag.p + q.n, sizeof(int), hipMemcpyDeviceToHost, st));
        DCHK(hipStreamSynchronize(st));
    }
    if (left < 0 || left > q.n) { err = "drifters_mask: the scan returned an impossible count"; return NXS_ERR_INTERNAL; }
    q.cur = b; q.n = left;
    if (n_left) *n_left = left;
    return NXS_OK;
}

int get(State *s, hipStream_t st, int set, int32_t *n, double *x, double *y, int32_t *id, double *conc, int32_t *found, std::string &err) {
    if (int rc = existing_set(s, set, err)) return rc;
    Set &q = s->sets[set];
    if (n) *n = q.n;
    if (q.n == 0) return NXS_OK;
    const int c = q.cur;
    const size_t nd = (size_t)q.n * sizeof(double), ni = (size_t)q.n * sizeof(int);
    if (x) DCHK(hipMemcpyAsync(x, q.x[c].p, nd, hipMemcpyDeviceToHost, st));
    if (y) DCHK(hipMemcpyAsync(y, q.y[c].p, nd, hipMemcpyDeviceToHost, st));
    if (id) DCHK(hipMemcpyAsync(id, q.id[c].p, ni, hipMemcpyDeviceToHost, st));
    if (conc) DCHK(hipMemcpyAsync(conc, q.conc[c].p, nd, hipMemcpyDeviceToHost, st));
    if (found) DCHK(hipMemcpyAsync(found, q.found[c].p, ni, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    return NXS_OK;
}

#undef DCHK

}  // namespace nxs_drifters
