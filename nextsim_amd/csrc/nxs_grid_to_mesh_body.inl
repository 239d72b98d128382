// nxs_grid_to_mesh_body.inl -- the arithmetic of InterpFromGridToMeshx (contrib/bamg/src/InterpFromGridToMeshx.cpp:14-485) for ONE target point: the ONE copy of it.
// Textually included by nxs_interp.hip (k_grid_to_mesh behind nxs_interp_grid_to_mesh: interleaved [nods][N_data] output) and by nxs_thermo_forcing_kernels.inl
// (k_thermo_forcing_ingest behind nxs_dyn_thermo_forcing_ingest: one [Ne] row per column), and by tests/thermo_forcing_host_kernel.cpp, which compiles it for the host
// with the HIP qualifiers defined away.  The two kernels differ only in WHERE a column's value goes: the `Store` argument (wants(j): is column j asked for; put(j, v)).
// Operand order is the reference's; the build is uncontracted (-ffp-contract=off).  Needs NXS_INTERP_* (include/nxs_interp.h).

struct G2M {
    const double *x, *y;  // pixel centres, x_rows / y_rows entries
    int x_rows, y_rows, M, N, N_data, nods, interp, row_major, mono_x, mono_y;
    double default_value;
};

// findindices (InterpFromGridToMeshx.cpp:361-395): the FIRST interval that brackets v, either orientation; the last
// coordinate itself belongs to the last interval.  On a strictly monotone axis that interval is unique: bisection.
__device__ __forceinline__ bool find_interval(const double *a, int rows, int mono, double v, int &idx) {
    bool found = false;
    idx = -1;
    if (mono != 0) {
        const bool asc = mono > 0;
        int lo = 0, hi = rows - 1;  // invariant: the bracketing interval, if any, lies in [lo, hi]
        if (asc ? (v >= a[0] && v < a[rows - 1]) : (v <= a[0] && v > a[rows - 1])) {
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (asc ? (a[mid] <= v) : (a[mid] >= v)) lo = mid; else hi = mid;
            }
            idx = lo;
            found = true;
        }
    } else {
        for (int i = 0; i < rows - 1; ++i)
            if (((a[i] <= v) && (v < a[i + 1])) || ((a[i] >= v) && (v > a[i + 1]))) { idx = i; found = true; break; }
    }
    if (v == a[rows - 1]) { idx = rows - 2; found = true; }
    return found;
}

// One target point (xg, yg): the grid interval is found once, then every wanted column takes the triangle / bilinear / nearest formula; NaN and a point outside the
// grid give default_value.
template <class Store>
__device__ __forceinline__ void grid_to_mesh_point(const G2M &g, const double *__restrict__ data, double xg, double yg, const Store &store) {
    int n, m;
    const bool fx = find_interval(g.x, g.x_rows, g.mono_x, xg, n), fy = find_interval(g.y, g.y_rows, g.mono_y, yg, m);
    if (!(fx && fy)) {
        for (int j = 0; j < g.N_data; ++j) if (store.wants(j)) store.put(j, g.default_value);
        return;
    }
    int n_min, n_max, m_min, m_max;
    if (g.x[n] < g.x[n + 1]) { n_min = n; n_max = n + 1; } else { n_min = n + 1; n_max = n; }
    if (g.y[m] < g.y[m + 1]) { m_min = m; m_max = m + 1; } else { m_min = m + 1; m_max = m; }
    const double x1 = g.x[n_min], x2 = g.x[n_max], y1 = g.y[m_min], y2 = g.y[m_max];
    const size_t ND = (size_t)g.N_data;
    for (int j = 0; j < g.N_data; ++j) {
        if (!store.wants(j)) continue;
        double Q11, Q12, Q21, Q22;
        if (g.row_major) {
            Q11 = data[ND * ((size_t)n_min * g.M + m_min) + j]; Q12 = data[ND * ((size_t)n_min * g.M + m_max) + j];
            Q21 = data[ND * ((size_t)n_max * g.M + m_min) + j]; Q22 = data[ND * ((size_t)n_max * g.M + m_max) + j];
        } else {
            Q11 = data[ND * ((size_t)m_min * g.N + n_min) + j]; Q12 = data[ND * ((size_t)m_max * g.N + n_min) + j];
            Q21 = data[ND * ((size_t)m_min * g.N + n_max) + j]; Q22 = data[ND * ((size_t)m_max * g.N + n_max) + j];
        }
        double v;
        if (g.interp == NXS_INTERP_TRIANGLE) {  // triangleinterp, :397-430
            const double area = (x2 - x1) * (y2 - y1);
            if ((xg - x1) / (x2 - x1) < (yg - y1) / (y2 - y1)) {
                const double area_1 = ((y2 - yg) * (x2 - x1)) / area, area_2 = ((xg - x1) * (y2 - y1)) / area, area_3 = 1 - area_1 - area_2;
                v = area_1 * Q11 + area_2 * Q22 + area_3 * Q12;
            } else {
                const double area_1 = ((yg - y1) * (x2 - x1)) / area, area_2 = ((x2 - xg) * (y2 - y1)) / area, area_3 = 1 - area_1 - area_2;
                v = area_1 * Q22 + area_2 * Q11 + area_3 * Q21;
            }
        } else if (g.interp == NXS_INTERP_BILINEAR) {  // bilinearinterp, :432-455
            v = +Q11 * (x2 - xg) * (y2 - yg) / ((x2 - x1) * (y2 - y1)) + Q21 * (xg - x1) * (y2 - yg) / ((x2 - x1) * (y2 - y1)) +
                Q12 * (x2 - xg) * (yg - y1) / ((x2 - x1) * (y2 - y1)) + Q22 * (xg - x1) * (yg - y1) / ((x2 - x1) * (y2 - y1));
        } else {  // nearestinterp, :457-485 -- xm, ym are HALF EXTENTS compared with absolute coordinates, as the reference does
            const double xmid = (x2 - x1) / 2, ymid = (y2 - y1) / 2;
            if (xg <= xmid && yg <= ymid) v = Q11;
            else if (xg <= xmid && yg > ymid) v = Q12;
            else if (xg > xmid && yg <= ymid) v = Q21;
            else v = Q22;
        }
        if (isnan(v)) v = g.default_value;
        store.put(j, v);
    }
}

// ---- host: what both entry points do before the launch
static inline int g2m_monotone(const double *a, int n) {
    bool asc = true, desc = true;
    for (int i = 0; i + 1 < n; ++i) { asc = asc && a[i] < a[i + 1]; desc = desc && a[i] > a[i + 1]; }
    return asc ? 1 : desc ? -1 : 0;
}
// the pixel centres: given (x_rows == N, y_rows == M), or taken from the contours (one more entry each, :44-53).  false: neither
static inline bool g2m_centres(const double *x_in, int x_rows, const double *y_in, int y_rows, int M, int N, double *x, double *y) {
    if (N == (x_rows - 1) && M == (y_rows - 1)) {
        for (int i = 0; i < N; ++i) x[i] = (x_in[i] + x_in[i + 1]) / 2.;
        for (int i = 0; i < M; ++i) y[i] = (y_in[i] + y_in[i + 1]) / 2.;
    } else if (N == x_rows && M == y_rows) {
        for (int i = 0; i < N; ++i) x[i] = x_in[i];
        for (int i = 0; i < M; ++i) y[i] = y_in[i];
    } else {
        return false;
    }
    return true;
}
