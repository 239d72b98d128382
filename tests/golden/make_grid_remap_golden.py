"""Generates tests/golden/bamg_grid_remap.npz: the conservative remapping between a mesh and a grid of quadrilateral cells, computed by the REAL
contrib/bamg -- ConservativeRemappingWeights, ConservativeRemappingMeshToGrid, ConservativeRemappingGridToMesh
(contrib/bamg/src/ConservativeRemapping.cpp:15-171) -- through a small door of our own, which is written into a temporary directory and compiled
against the reference's headers and oracle/_ref/libbamg_ref.so.  Run in the build container (needs /root/reference, oracle/_ref and g++):

    python tests/golden/make_grid_remap_golden.py

The door builds the BamgMesh with BamgConvertMeshx (as oracle/bamg_shim.cpp does), calls the weights routine and restates the compaction GridOutput
does with its output (model/gridoutput.cpp:706-735: the entries of local triangles renumbered, rows left empty dropped) -- without a filter (every
triangle is local: the land rows go) and with one (`local_of_root`, -1 = not here).  The two applications are called on the COMPACT lists, as
GridOutput and the coupling datasets call them.

Only the .npz travels (the reference does not exist on the GPU box).  cases() is pure numpy: tests/test_grid_remap_host.py regenerates the file where
the reference is present and requires identical bytes of every array.

Per case NAME the file holds  NAME_x, _y [nods], _tri [nels][3] (0-based), _gridX, _gridY [G], _cornerX, _cornerY [G][4];
  _gridP [R], _off [R+1], _tris, _w [off[R]]            the compact lists (wet rows only)
  _local [nels], _r_gridP, _r_off, _r_tris, _r_w        the filter and the lists it leaves
  _m2g_in{1,7} [nels][nv], _m2g_out{1,7} [G][nv]        ConservativeRemappingMeshToGrid with miss_val = MISS
  _g2m_in{1,7} [G][nv],   _g2m_out{1,7} [nels][nv]      ConservativeRemappingGridToMesh
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NXS_REFERENCE", "/root/reference")
DST = os.path.join(HERE, "bamg_grid_remap.npz")
MISS = 1e14
H = 1000.   # spacing of the structured triangulations, metres (the reference's tolerances are absolute: 1e-3, 1e-8, 1e-6)

DOOR = r'''
#include <cstring>
#include <vector>
#include "BamgMesh.h"
#include "BamgGeom.h"
#include "BamgConvertMeshx.h"
#include "ConservativeRemapping.hpp"

typedef std::vector<std::vector<int>> Lists;
typedef std::vector<std::vector<double>> Weights;

static void unpack(int rows, const int *off, const int *tris, const double *w, Lists &t, Weights &ww) {
    t.resize(rows); ww.resize(rows);
    for (int i = 0; i < rows; ++i) { t[i].assign(tris + off[i], tris + off[i + 1]); ww[i].assign(w + off[i], w + off[i + 1]); }
}

extern "C" {

/* ConservativeRemappingWeights on the mesh, then the compaction of gridoutput.cpp:706-735 (local_of_root == NULL: every triangle is local under its own
 * number).  Returns the number of rows, -1 when BamgConvertMeshx fails, -2 - needed when cap is too small. */
int door_weights(const int *index, const double *x, const double *y, int nods, int nels, const double *gridX, const double *gridY,
                 const double *cornerX, const double *cornerY, int G, const int *local_of_root, int *gridP_out, int *off_out, int cap,
                 int *tris_out, double *w_out, int *longest_raw) {
    BamgMesh *mesh = new BamgMesh();
    BamgGeom *geom = new BamgGeom();
    int rc = BamgConvertMeshx(mesh, geom, const_cast<int *>(index), const_cast<double *>(x), const_cast<double *>(y), nods, nels);
    if (rc != 1 || mesh->TrianglesSize[0] != nels) { delete geom; delete mesh; return -1; }
    std::vector<double> gx(gridX, gridX + G), gy(gridY, gridY + G), cx(cornerX, cornerX + 4 * G), cy(cornerY, cornerY + 4 * G);
    std::vector<int> gridP;
    Lists triangles;
    Weights weights;
    ConservativeRemappingWeights(mesh, gx, gy, cx, cy, gridP, triangles, weights);
    delete geom; delete mesh;
    int rows = 0, n = 0, longest = 0;
    for (size_t i = 0; i < gridP.size(); ++i) {
        if ((int)triangles[i].size() > longest) longest = (int)triangles[i].size();
        const int first = n;
        for (size_t j = 0; j < triangles[i].size(); ++j) {
            const int tr = triangles[i][j];
            const int loc = local_of_root ? local_of_root[tr] : tr;
            if (loc < 0) continue;
            if (n < cap) { tris_out[n] = loc; w_out[n] = weights[i][j]; }
            ++n;
        }
        if (n > first) { gridP_out[rows] = gridP[i]; off_out[rows] = first; ++rows; }
    }
    off_out[rows] = n;
    if (longest_raw) *longest_raw = longest;
    return n > cap ? -2 - n : rows;
}

int door_mesh_to_grid(const double *in, int nels, int nb_var, int G, double miss_val, int rows, const int *gridP, const int *off, const int *tris,
                      const double *w, const double *cornerX, const double *cornerY, double *out) {
    Lists t; Weights ww;
    unpack(rows, off, tris, w, t, ww);
    std::vector<int> gp(gridP, gridP + rows);
    std::vector<double> vin(in, in + (size_t)nels * nb_var), cx(cornerX, cornerX + 4 * G), cy(cornerY, cornerY + 4 * G);
    double *res = NULL;
    ConservativeRemappingMeshToGrid(res, vin, nb_var, G, miss_val, gp, cx, cy, t, ww);
    std::memcpy(out, res, sizeof(double) * (size_t)G * nb_var);
    delete[] res;
    return 0;
}

int door_grid_to_mesh(const double *in, int G, int nb_var, int nels, int rows, const int *gridP, const int *off, const int *tris, const double *w,
                      double *out) {
    Lists t; Weights ww;
    unpack(rows, off, tris, w, t, ww);
    std::vector<int> gp(gridP, gridP + rows);
    std::vector<double> vin(in, in + (size_t)G * nb_var);
    double *res = NULL;
    ConservativeRemappingGridToMesh(res, vin, nb_var, nels, gp, t, ww);
    std::memcpy(out, res, sizeof(double) * (size_t)nels * nb_var);
    delete[] res;
    return 0;
}

}
'''


def mesh(nx, ny, seed):
    """nx x ny nodes at spacing H, interior nodes moved by up to +-0.25 H; every quad cut along the same diagonal, counter-clockwise."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    x, y = H * i.astype(np.float64), H * j.astype(np.float64)
    inner = (i > 0) & (i < nx - 1) & (j > 0) & (j < ny - 1)
    x = x + np.where(inner, rng.uniform(-0.25 * H, 0.25 * H, x.shape), 0.)
    y = y + np.where(inner, rng.uniform(-0.25 * H, 0.25 * H, y.shape), 0.)
    a = (j[:-1, :-1] * nx + i[:-1, :-1]).ravel()
    tri = np.empty((2 * a.size, 3), np.int32)
    tri[0::2] = np.column_stack([a, a + 1, a + nx + 1])
    tri[1::2] = np.column_stack([a, a + nx + 1, a + nx])
    return np.ascontiguousarray(x.ravel()), np.ascontiguousarray(y.ravel()), tri


def grid(n, m, d, angle, cx, cy, origin=None):
    """n x m cells of side d, turned by `angle` about (cx, cy) and centred there -- or, with `origin`, unrotated from that corner.  Corners
    counter-clockwise from the lower left; the P-point is the middle of the cell."""
    jj, ii = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    u0 = (ii.ravel() - 0.5 * n) * d if origin is None else origin[0] + ii.ravel() * d - cx
    v0 = (jj.ravel() - 0.5 * m) * d if origin is None else origin[1] + jj.ravel() * d - cy
    cu = np.stack([u0, u0 + d, u0 + d, u0], 1); cv = np.stack([v0, v0, v0 + d, v0 + d], 1)
    co, si = np.cos(angle), np.sin(angle)

    def turn(u, v):
        return (cx + (co * u - si * v), cy + (si * u + co * v)) if angle else (cx + u, cy + v)
    X, Y = turn(cu, cv)
    px, py = turn(u0 + 0.5 * d, v0 + 0.5 * d)
    return np.ascontiguousarray(px), np.ascontiguousarray(py), np.ascontiguousarray(X), np.ascontiguousarray(Y)


def field(rows, nv, seed):
    """Multiples of 1/64 in [-8, 8] (they compress; the weights they meet are full doubles), with -0., +Inf, -Inf and one NaN in every column."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-512, 513, (rows, nv)).astype(np.float64) / 64.
    if rows >= 4:
        for v in range(nv):
            r = rng.choice(rows, 4, replace=False)
            a[r[0], v] = -0.; a[r[1], v] = np.inf; a[r[2], v] = -np.inf; a[r[3], v] = np.nan
    return a


def cases():
    out = {}

    def add(name, nx, ny, seed, g):
        x, y, tri = mesh(nx, ny, seed)
        cen = x[tri].sum(1) / 3.
        here = cen < 0.5 * (x.min() + x.max())      # the `local_of_root` filter: the western half, renumbered in order
        local = np.where(here, np.cumsum(here) - 1, -1).astype(np.int32)
        out[name] = dict(x=x, y=y, tri=tri, gridX=g[0], gridY=g[1], cornerX=g[2], cornerY=g[3], local=local)

    mx, my = 6000., 5000.
    add("coarse", 13, 11, 1, grid(6, 6, 3700., 0.3, mx, my))
    add("long_rows", 40, 33, 2, grid(6, 6, 12500., 0.2, 19500., 16000.))
    add("fine", 9, 7, 3, grid(21, 21, 700., 0.1, 4000., 3000.))
    add("aligned", 13, 10, 4, grid(6, 5, 3000., 0., 0., 0., origin=(-3000., -3000.)))
    add("all_land", 13, 11, 1, grid(3, 3, 3700., 0.3, mx + 60000., my))
    add("one_cell", 13, 11, 1, grid(1, 1, 3700., 0.3, mx, my))
    add("inside", 9, 7, 3, grid(12, 12, 250., 0.1, 4000., 3000.))   # cells smaller than the triangles: "the whole cell is in the triangle"
    for k, (name, c) in enumerate(out.items()):
        nels, G = c["tri"].shape[0], c["gridX"].size
        for nv in (1, 7):
            c[f"m2g_in{nv}"] = field(nels, nv, 100 + 10 * k + nv)
            c[f"g2m_in{nv}"] = field(G, nv, 200 + 10 * k + nv)
    return out


def build_door(tmp):
    src, lib = os.path.join(tmp, "door.cpp"), os.path.join(tmp, "libdoor.so")
    open(src, "w").write(DOOR)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-w", "-D_MULTITHREADING_", "-DNDEBUG", "-I" + os.path.join(REF, "contrib", "bamg", "include"),
                           "-shared", "-o", lib, src, "-L" + refdir, "-lbamg_ref", "-Wl,-rpath," + refdir, "-lgomp"])
    return C.CDLL(lib)


def compute(L):
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ip = lambda a: a.ctypes.data_as(IP)   # noqa: E731
    dp = lambda a: a.ctypes.data_as(DP)   # noqa: E731
    L.door_mesh_to_grid.argtypes = [DP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, IP, IP, IP, DP, DP, DP, DP]
    arrays, counts = {}, {}
    for name, c in cases().items():
        x, y, tri = c["x"], c["y"], c["tri"]
        idx = np.ascontiguousarray((tri + 1).ravel().astype(np.intc))
        G, nels = c["gridX"].size, tri.shape[0]
        cX, cY = np.ascontiguousarray(c["cornerX"].ravel()), np.ascontiguousarray(c["cornerY"].ravel())

        def weights(local):
            cap = 64 * nels + 64
            gp, off = np.zeros(G, np.intc), np.zeros(G + 1, np.intc)
            tr, w = np.zeros(cap, np.intc), np.zeros(cap)
            longest = C.c_int(0)
            rows = L.door_weights(ip(idx), dp(x), dp(y), x.size, nels, dp(c["gridX"]), dp(c["gridY"]), dp(cX), dp(cY), G,
                                  None if local is None else ip(np.ascontiguousarray(local.astype(np.intc))), ip(gp), ip(off), cap, ip(tr), dp(w), C.byref(longest))
            assert rows >= 0, (name, rows)
            n = int(off[rows])
            return gp[:rows].astype(np.int32), off[:rows + 1].astype(np.int32), tr[:n].astype(np.int32), w[:n].copy(), longest.value

        gp, off, tr, w, longest = weights(None)
        r = weights(c["local"])
        for k in ("x", "y", "tri", "gridX", "gridY", "cornerX", "cornerY", "local"):
            arrays[f"{name}_{k}"] = c[k]
        arrays.update({f"{name}_gridP": gp, f"{name}_off": off, f"{name}_tris": tr, f"{name}_w": w,
                       f"{name}_r_gridP": r[0], f"{name}_r_off": r[1], f"{name}_r_tris": r[2], f"{name}_r_w": r[3]})
        gpc, offc, trc = (np.ascontiguousarray(a.astype(np.intc)) for a in (gp, off, tr))
        for nv in (1, 7):
            a = np.ascontiguousarray(c[f"m2g_in{nv}"]); o = np.empty((G, nv))
            assert L.door_mesh_to_grid(dp(a), nels, nv, G, MISS, gp.size, ip(gpc), ip(offc), ip(trc), dp(w), dp(cX), dp(cY), dp(o)) == 0
            arrays[f"{name}_m2g_in{nv}"] = a; arrays[f"{name}_m2g_out{nv}"] = o
            b = np.ascontiguousarray(c[f"g2m_in{nv}"]); o2 = np.empty((nels, nv))
            assert L.door_grid_to_mesh(dp(b), G, nv, nels, gp.size, ip(gpc), ip(offc), ip(trc), dp(w), dp(o2)) == 0
            arrays[f"{name}_g2m_in{nv}"] = b; arrays[f"{name}_g2m_out{nv}"] = o2
        counts[name] = dict(wet=int(gp.size), entries=int(tr.size), longest=int(np.diff(off).max()) if gp.size else 0, longest_raw=longest,
                            touched=int(np.unique(tr).size), nels=nels, G=G)
    return arrays, counts


def make(dst=DST):
    with tempfile.TemporaryDirectory() as tmp:
        arrays, counts = compute(build_door(tmp))
    np.savez_compressed(dst, **arrays)
    return counts


if __name__ == "__main__":
    for name, c in make().items():
        print(name, c)
    print(DST, os.path.getsize(DST), "bytes")
    sys.exit(0)
