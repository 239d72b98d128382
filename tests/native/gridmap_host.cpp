// gridmap_host.cpp -- TEST PROGRAM (tests/test_grid_remap_host.py).  The per-cell functions nxs_gridmap_create runs on the device
// (nextsim_amd/csrc/nxs_remap_core.inl with NC = 4) compiled for the host, with plain loops around them for what the kernels of
// nxs_gridmap_kernels.inl do: the walk per wet cell, the compaction into lists, the filter of nxs_gridmap_restrict, the transposition and the
// two applications.  So the transcription of ConservativeRemappingWeights / MeshToGrid / GridToMesh is checked against the real bamg's bits
// (tests/golden/bamg_grid_remap.npz) without a device, and -- built a second time with -fsanitize=address,undefined -- for out-of-bounds
// accesses of the walk.  The seeds (the element holding each P-point, -1 = land) come with the input: the exact locator is device code.
//
//   gridmap_host IN OUT
//   IN : int32 nods, nels, nec_w, G, nb_var, has_local, cap, 0; tri[3 nels]; nec[nods nec_w]; ec[3 nels]; seed[G]; local[nels] (if has_local);
//        double x[nods], y[nods], cornerX[4 G], cornerY[4 G], m2g_in[nels nb_var], g2m_in[G nb_var], miss_val
//   OUT: int32 rows, n, failed, longest; gridP[rows]; off[rows + 1]; tris[n]; double w[n];
//        int32 r_rows, r_n; r_gridP; r_off; r_tris; double r_w;   (zeros without a filter)
//        double m2g_out[G nb_var], g2m_out[nels nb_var]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define NXS_HD
#include "nxs_remap_core.inl"

template <typename T>
static std::vector<T> get(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <typename T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: gridmap_host IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = get<int32_t>(f, 8);
    const int nods = hd[0], nels = hd[1], nec_w = hd[2], G = hd[3], nb_var = hd[4], has_local = hd[5], cap = hd[6];
    const auto tri = get<int32_t>(f, 3 * (size_t)nels), nec = get<int32_t>(f, (size_t)nods * nec_w), ec = get<int32_t>(f, 3 * (size_t)nels);
    const auto seed = get<int32_t>(f, G), local = get<int32_t>(f, has_local ? nels : 0);
    const auto x = get<double>(f, nods), y = get<double>(f, nods), cX = get<double>(f, 4 * (size_t)G), cY = get<double>(f, 4 * (size_t)G);
    const auto m2g_in = get<double>(f, (size_t)nels * nb_var), g2m_in = get<double>(f, (size_t)G * nb_var);
    const double miss_val = get<double>(f, 1)[0];
    fclose(f);

    const nxs_remap::OldMesh m{nels, nods, tri.data(), x.data(), y.data(), nec.data(), nec_w, ec.data()};
    // ---- the walk per wet cell and the compaction (k_gridmap_walk, k_gridmap_compact): wet rows only, failed cells dropped and counted
    std::vector<int32_t> gridP, off(1, 0), tris;
    std::vector<double> w, r_area;
    std::vector<int> lt(cap);
    std::vector<double> lw(cap);
    std::vector<nxs_remap::Frame> stack(cap + 1);
    int failed = 0, longest = 0;
    for (int c = 0; c < G; ++c) {
        if (seed[c] < 0) continue;
        const int n = nxs_remap::collect_n<4>(m, &cX[4 * (size_t)c], &cY[4 * (size_t)c], seed[c], false, lt.data(), lw.data(), stack.data(), cap);
        if (n < 0) { ++failed; continue; }
        gridP.push_back(c);
        tris.insert(tris.end(), lt.begin(), lt.begin() + n);
        w.insert(w.end(), lw.begin(), lw.begin() + n);
        off.push_back((int32_t)tris.size());
        r_area.push_back(nxs_remap::r_cell_area_n<4>(&cX[4 * (size_t)c], &cY[4 * (size_t)c]));
        if (n > longest) longest = n;
    }
    const int rows = (int)gridP.size();
    // ---- nxs_gridmap_restrict: the entries of local triangles, renumbered; rows left empty dropped (gridoutput.cpp:706-735)
    std::vector<int32_t> r_gridP, r_off(1, 0), r_tris;
    std::vector<double> r_w;
    if (has_local)
        for (int i = 0; i < rows; ++i) {
            for (int k = off[i]; k < off[i + 1]; ++k)
                if (local[tris[k]] >= 0) { r_tris.push_back(local[tris[k]]); r_w.push_back(w[k]); }
            if ((int)r_tris.size() > r_off.back()) { r_gridP.push_back(gridP[i]); r_off.push_back((int32_t)r_tris.size()); }
        }
    // ---- mesh -> grid (k_gridmap_to_grid): every cell miss_val, a wet one its row's sum
    std::vector<double> m2g((size_t)G * nb_var, miss_val), g2m((size_t)nels * nb_var);
    for (int i = 0; i < rows; ++i)
        for (int v = 0; v < nb_var; ++v)
            m2g[(size_t)gridP[i] * nb_var + v] = nxs_remap::grid_value(m2g_in.data(), nb_var, v, tris.data() + off[i], w.data() + off[i], off[i + 1] - off[i], r_area[i]);
    // ---- the transposition (k_gridmap_t_count / _fill, then every row sorted): per triangle the indices of its entries, ascending
    std::vector<int32_t> t_off(nels + 1, 0), cell(tris.size());
    for (int32_t t : tris) ++t_off[t + 1];
    for (int t = 0; t < nels; ++t) t_off[t + 1] += t_off[t];
    std::vector<int32_t> t_pos(tris.size()), cursor(t_off.begin(), t_off.end() - 1);
    for (int i = 0; i < rows; ++i)
        for (int k = off[i]; k < off[i + 1]; ++k) { t_pos[cursor[tris[k]]++] = k; cell[k] = gridP[i]; }
    // ---- grid -> mesh as a gather (k_gridmap_to_mesh)
    for (int t = 0; t < nels; ++t)
        for (int v = 0; v < nb_var; ++v)
            g2m[(size_t)t * nb_var + v] = nxs_remap::mesh_value(g2m_in.data(), nb_var, v, t_pos.data() + t_off[t], t_off[t + 1] - t_off[t], cell.data(), w.data());

    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    put<int32_t>(o, {rows, (int32_t)tris.size(), failed, longest});
    put(o, gridP); put(o, off); put(o, tris); put(o, w);
    put<int32_t>(o, {(int32_t)r_gridP.size(), (int32_t)r_tris.size()});
    put(o, r_gridP); put(o, r_off); put(o, r_tris); put(o, r_w);
    put(o, m2g); put(o, g2m);
    fclose(o);
    return 0;
}
