"""A Python restatement of GridOutput::updateGridMean() on the REGULAR grid (model/gridoutput.cpp:387-415, the M_is_regular_grid branch of updateGridMeanWorker
:486-505, :511-538), of setProcMask (:360-378), rotateVectors (:578-623), setLSM (:558-574), applyLSM (:639-651) -- what nxs_dyn_means_regular_* computes -- and of
contrib/bamg/src/InterpFromMeshToGridx.cpp.  The three InterpFromMeshToGridx calls are a function argument with the signature of the door to the real library,
oracle.pyoracle.bamg_interp_mesh_to_grid: the restated one below is the default, tests/golden/make_means_regular_golden.py passes the REAL contrib/bamg instead.
bamg's "nrows" is M_ncols (along x) and its "ncols" is M_nrows (along y): the output is [M_ncols, M_nrows, N_data], the bamg index of the point (i, j) is
b = i * M_nrows + j and its grid index g = i + M_ncols * j.  rotateVectors indexes interp_out AND gridLON by b, although gridLON was filled by g: restated as it stands
(cosang[k] / sinang[k] come from gridLON[k] and multiply row k of interp_out in bamg order).
cos / sin go through math.cos / math.sin (means_points_ref.cos_sin): the libm the library's host code calls.  Everything else is elementwise IEEE arithmetic that
numpy does as C does, one rounding per operation.  Shared by the CPU and GPU tests of the feature."""
from __future__ import annotations

import math

import numpy as np

import means_points_ref as P

PI = P.PI
equal, same_bits, cos_sin, apply_lsm = P.equal, P.same_bits, P.cos_sin, P.apply_lsm


def grid_axes(xmin, ymax, xposting, yposting, nrows, ncols):
    """x_grid, y_grid of InterpFromMeshToGridx.cpp:72-91 (both flips)."""
    x_grid, y_grid = np.zeros(nrows), np.zeros(ncols)
    i = np.arange(nrows, dtype=np.float64)
    if xposting < 0:
        x_grid[::-1] = xmin - xposting * i
    else:
        x_grid[:] = xmin + xposting * i
    i = np.arange(ncols, dtype=np.float64)
    if yposting < 0:
        y_grid[:] = ymax + yposting * i
    else:
        y_grid[::-1] = ymax - yposting * i
    return x_grid, y_grid


def interp_mesh_to_grid(index_mesh, x_mesh, y_mesh, data, xmin, ymax, xposting, yposting, nrows, ncols, default_value, winners=None):
    """InterpFromMeshToGridx, line by line: -> [nrows, ncols, N_data].  index_mesh is 1-based, [3 nels].  winners ([nrows, ncols] int, optional) receives the element
    whose values each point ended up with (-1: none)."""
    idx = np.asarray(index_mesh, np.int64).reshape(-1, 3) - 1
    nels, nods = idx.shape[0], x_mesh.size
    data = np.asarray(data, np.float64)
    data = data[:, None] if data.ndim == 1 else data
    N = data.shape[1]
    assert nels >= 1 and nods >= 3 and ncols >= 1 and nrows >= 1 and xposting != 0 and yposting != 0                      # :33
    assert data.shape[0] in (nods, nels)
    nodal = data.shape[0] == nods                                                                                         # :38 (the node count is asked first)
    griddata = np.full((nrows, ncols, N), float(default_value))
    x_grid, y_grid = grid_axes(xmin, ymax, xposting, yposting, nrows, ncols)
    xflip, yflip = xposting < 0, yposting < 0
    x_grid_min, x_grid_max = (x_grid[-1], x_grid[0]) if xflip else (x_grid[0], x_grid[-1])
    y_grid_min, y_grid_max = (y_grid[-1], y_grid[0]) if yflip else (y_grid[0], y_grid[-1])
    X, Y = x_mesh[idx], y_mesh[idx]
    txmin, txmax, tymin, tymax = X.min(1), X.max(1), Y.min(1), Y.max(1)
    with np.errstate(all="ignore"):
        for n in np.flatnonzero(~((txmin > x_grid_max) | (txmax < x_grid_min) | (tymin > y_grid_max) | (tymax < y_grid_min))):      # :111
            x1, x2, x3 = (float(v) for v in X[n])
            y1, y2, y3 = (float(v) for v in Y[n])
            if xflip:
                i1 = max(0, int(math.floor((txmax[n] - x_grid_max) / xposting)) - 1); i2 = min(nrows - 1, int(math.ceil((txmin[n] - x_grid_max) / xposting)))
            else:
                i1 = max(0, int(math.floor((txmin[n] - x_grid_min) / xposting)) - 1); i2 = min(nrows - 1, int(math.ceil((txmax[n] - x_grid_min) / xposting)))
            if yflip:
                j1 = max(0, int(math.floor((tymax[n] - y_grid_max) / yposting)) - 1); j2 = min(ncols - 1, int(math.ceil((tymin[n] - y_grid_max) / yposting)))
            else:
                j1 = max(0, int(math.floor((tymin[n] - y_grid_min) / yposting)) - 1); j2 = min(ncols - 1, int(math.ceil((tymax[n] - y_grid_min) / yposting)))
            if i2 < i1 or j2 < j1:
                continue
            area = x2 * y3 - y2 * x3 + x1 * y2 - y1 * x2 + x3 * y1 - y3 * x1                                                  # :135-137
            xg, yg = x_grid[i1:i2 + 1][:, None], y_grid[j1:j2 + 1][None, :]
            inbox = ~((xg > txmax[n]) | (xg < txmin[n])) & ~((yg > tymax[n]) | (yg < tymin[n]))                              # :143, :148
            area_1 = ((xg - x3) * (y2 - y3) - (yg - y3) * (x2 - x3)) / np.float64(area)
            area_2 = ((x1 - x3) * (yg - y3) - (y1 - y3) * (xg - x3)) / np.float64(area)
            area_3 = 1 - area_1 - area_2
            ok = inbox & (area_1 > -10e-12) & (area_2 > -10e-12) & (area_3 > -10e-12)
            if not ok.any():
                continue
            if nodal:
                value = area_1[..., None] * data[idx[n, 0]]
                value = value + area_2[..., None] * data[idx[n, 1]]
                value = value + area_3[..., None] * data[idx[n, 2]]
            else:
                value = np.broadcast_to(data[n], ok.shape + (N,))
            value = np.where(np.isnan(value), float(default_value), value)                                                   # :175
            griddata[i1:i2 + 1, j1:j2 + 1][ok] = value[ok]
            if winners is not None:
                winners[i1:i2 + 1, j1:j2 + 1][ok] = n
    return griddata


def find_winners(x, y, tri, g, interp=interp_mesh_to_grid):
    """The element every grid point ends up with, in GRID order (-1: none), read off an interpolation of the element numbers."""
    ne = tri.shape[0]
    assert ne != x.size                                                      # (the library tells elemental data from nodal data by the length)
    out = interp((tri + 1).ravel(), x, y, np.arange(ne, dtype=np.float64), g["xmin"], g["ymax"], g["spacing"], g["spacing"], g["ncols"], g["nrows"], -1.)
    return to_grid_order(out.reshape(-1, 1), g)[:, 0].astype(np.int32)


def bamg_of_grid(g):
    """b(g): the bamg index of every grid index."""
    return (np.arange(g["ncols"])[None, :] * g["nrows"] + np.arange(g["nrows"])[:, None]).ravel()


def to_grid_order(out, g):
    """interp_out [G, N] in bamg order -> grid order (gridoutput.cpp:526-537)."""
    return out[bamg_of_grid(g)]


def grid_points(g):
    """The coordinates of the grid points in GRID order, from the axes as the library builds them."""
    x_grid, y_grid = grid_axes(g["xmin"], g["ymax"], g["spacing"], g["spacing"], g["ncols"], g["nrows"])
    return np.tile(x_grid, g["nrows"]), np.repeat(y_grid, g["ncols"])


def update_grid_mean(ge, gn, x, y, tri, n_owned, el, nod, g, pairs=(), cosang=None, sinang=None, miss_val=-1e14, ice_col=-1, el_mask=(), nod_mask=(),
                     interp=interp_mesh_to_grid):
    """updateGridMean(): ge [n_el, G] and gn [n_nod, G] in grid order (either None for an empty list) are added to IN PLACE; x, y = the DISPLACED nodes;
    el [Ne, n_el], nod [Nn, n_nod]; g = dict(xmin, ymax, spacing, ncols, nrows); cosang / sinang [G]: entry k from gridLON[k]."""
    ne, G = tri.shape[0], g["ncols"] * g["nrows"]
    n_el = 0 if ge is None else ge.shape[0]
    n_nod = 0 if gn is None else gn.shape[0]
    index = (tri + 1).ravel()

    def call(data):
        return np.array(interp(index, x, y, data, g["xmin"], g["ymax"], g["spacing"], g["spacing"], g["ncols"], g["nrows"], 0.)).reshape(G, -1)
    with np.errstate(invalid="ignore"):
        if n_nod:      # setProcMask (gridoutput.cpp:360-378, 391-395)
            ones = (np.arange(ne) < n_owned).astype(np.float64)
            proc_mask = np.zeros(G) + to_grid_order(call(ones), g)[:, 0]
        if n_el:
            out = to_grid_order(call(el), g)
            for nv in range(n_el):
                ge[nv] += out[:, nv]
        if n_nod:
            out = call(nod)
            P.rotate(out, pairs, cosang, sinang, miss_val)      # in BAMG order, cosang[k] on row k
            out = to_grid_order(out, g)
            for nv in range(n_nod):
                gn[nv] += out[:, nv] * proc_mask
        if ice_col >= 0:      # gridoutput.cpp:404-414
            for grid, masks in ((gn, nod_mask), (ge, el_mask)):
                for nv, m in enumerate(masks):
                    if m:
                        sel = (ge[ice_col] <= 0.) & (grid[nv] != miss_val)
                        grid[nv][sel] = 0.


def set_lsm(x, y, tri, g, interp=interp_mesh_to_grid):
    """setLSM: ones on every triangle of the mesh AT REST, default 0., converted to int; grid order."""
    out = np.array(interp((tri + 1).ravel(), x, y, np.ones(tri.shape[0]), g["xmin"], g["ymax"], g["spacing"], g["spacing"], g["ncols"], g["nrows"], 0.))
    return (np.zeros(g["ncols"] * g["nrows"]) + to_grid_order(out.reshape(-1, 1), g)[:, 0]).astype(np.int32)
