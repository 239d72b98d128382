"""A Python restatement of GridOutput::updateGridMean() on a LOADED grid without conservative remapping (model/gridoutput.cpp:387-415, 470-485, 511-545), of
rotateVectors (:578-623), setLSM (:558-574), applyLSM (:639-651) -- what nxs_dyn_means_points_* computes.  The three InterpFromMeshToMesh2dx calls (isdefault = true,
default 0.) are a function argument: the restated one below locates EXACTLY with tests/drifters_ref.locate (bamg's integer plane, 64-bit determinants) and
interpolates in the operand order of InterpFromMeshToMesh2dx.cpp:113-116, 157-170; tests/golden/make_means_points_golden.py passes the REAL contrib/bamg instead.
cos / sin go through math.cos / math.sin: the libm the library's host code calls (numpy's vectorised versions are another implementation).
Everything else is elementwise IEEE arithmetic that numpy does as C does, one rounding per operation.  Shared by the CPU and GPU tests of the feature."""
from __future__ import annotations

import math

import numpy as np

import drifters_ref as R

PI = 3.141592653589793      # contrib/mapx/include/mapx.h:47


def interp_located(x, y, tri, data, px, py, nodal):
    """InterpFromMeshToMesh2dx(..., isdefault = true, 0.) -> [n, N_data], with (it, dd) of the exact location."""
    data = np.asarray(data, np.float64)
    data = data[:, None] if data.ndim == 1 else data
    it, dd = R.locate(x, y, tri, px, py)
    out = np.zeros((px.size, data.shape[1]))
    m = np.flatnonzero(it >= 0)
    if nodal:
        det = (dd[m, 0] + dd[m, 1] + dd[m, 2]).astype(np.float64)
        a = [dd[m, k].astype(np.float64) / det for k in range(3)]
        i0, i1, i2 = tri[it[m], 0], tri[it[m], 1], tri[it[m], 2]
        with np.errstate(invalid="ignore"):
            out[m] = a[0][:, None] * data[i0] + a[1][:, None] * data[i1] + a[2][:, None] * data[i2]
    else:
        out[m] = data[it[m]]
    return out, it, dd


def interp(x, y, tri, data, px, py, nodal):
    return interp_located(x, y, tri, data, px, py, nodal)[0]


def cos_sin(rotation, rotation_angle, lon=None, theta=None):
    """cosang, sinang of gridoutput.cpp:602-614 (None, None for "none")."""
    if rotation == "none":
        return None, None
    if rotation == "north_east":
        ang = [rotation_angle - float(v) * PI / 180 for v in lon]
    else:
        ang = [rotation_angle - float(v) for v in theta]
    return np.array([math.cos(a) for a in ang]), np.array([math.sin(a) for a in ang])


def rotate(out, pairs, cosang, sinang, miss_val):
    """rotateVectors for every pair in list order, in place on interp_out [G, n_nod]."""
    if cosang is None:
        return
    for first, second in pairs:
        sel = out[:, first] != miss_val
        with np.errstate(invalid="ignore"):
            u = cosang * out[:, first] - sinang * out[:, second]
            v = sinang * out[:, first] + cosang * out[:, second]
        out[sel, first] = u[sel]
        out[sel, second] = v[sel]


def update_grid_mean(ge, gn, x, y, tri, n_owned, el, nod, gx, gy, pairs=(), cosang=None, sinang=None, miss_val=-1e14, ice_col=-1, el_mask=(), nod_mask=(), interp=interp):
    """updateGridMean(): ge [n_el, G] and gn [n_nod, G] (either None for an empty list) are added to IN PLACE; x, y = the DISPLACED nodes; el [Ne, n_el], nod [Nn, n_nod]."""
    ne = tri.shape[0]
    n_el = 0 if ge is None else ge.shape[0]
    n_nod = 0 if gn is None else gn.shape[0]
    with np.errstate(invalid="ignore"):
        if n_nod:      # setProcMask (gridoutput.cpp:360-378, 391-395)
            ones = (np.arange(ne) < n_owned).astype(np.float64)
            proc_mask = np.zeros(gx.size) + interp(x, y, tri, ones, gx, gy, False)[:, 0]
        if n_el:
            out = interp(x, y, tri, el, gx, gy, False)
            for nv in range(n_el):
                ge[nv] += out[:, nv]
        if n_nod:
            out = np.array(interp(x, y, tri, nod, gx, gy, True))
            rotate(out, pairs, cosang, sinang, miss_val)
            for nv in range(n_nod):
                gn[nv] += out[:, nv] * proc_mask
        if ice_col >= 0:      # gridoutput.cpp:404-414
            for g, masks in ((gn, nod_mask), (ge, el_mask)):
                for nv, m in enumerate(masks):
                    if m:
                        sel = (ge[ice_col] <= 0.) & (g[nv] != miss_val)
                        g[nv][sel] = 0.


def set_lsm(x, y, tri, gx, gy, interp=interp):
    """setLSM: ones on every triangle of the mesh AT REST, default 0., converted to int."""
    return (np.zeros(gx.size) + interp(x, y, tri, np.ones(tri.shape[0]), gx, gy, False)[:, 0]).astype(np.int32)


def apply_lsm(g, lsm, miss_val):
    out = g.copy()
    out[:, lsm == 0] = miss_val
    return out


def ties(x, y, tri, gx, gy):
    """How many grid points inside the mesh have a zero integer area coordinate (the one case in which the reference's own answer depends on its walk)."""
    it, dd = R.locate(x, y, tri, gx, gy)
    return int(((dd == 0).any(1) & (it >= 0)).sum())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def equal(a, b):
    """np.array_equal with NaN == NaN (the fixture holds a NaN node on purpose; a NaN's payload is not compared), and the same BITS everywhere else: -0. is not +0."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
