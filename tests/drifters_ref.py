"""A numpy restatement of the three statements of checkUpdateDrifters() that touch the model's arrays -- Drifters::move, Drifters::updateConc,
Drifters::maskXY (model/drifters.cpp:468-579) -- with InterpFromMeshToMesh2dx (isdefault = true, default 0.) located EXACTLY: bamg's integer plane
(Mesh::SetIntCoor, Mesh.cpp:3441-3468), 64-bit determinants (include/det.h), every triangle tried (brute force, ascending number), the operand order of
InterpFromMeshToMesh2dx.cpp:113-116, 151-156.  All integers stay below 2^62, so int64 arithmetic is exact.  Shared by the CPU and GPU drifter tests."""
from __future__ import annotations

import numpy as np


def mesh_bbox(x, y):
    return np.array([x.min(), x.max(), y.min(), y.max()])


def int_plane(x, y, bbox=None):
    """ix, iy (int64) of the vertices and the plane (coef, pminx, pminy, box); bbox = xmin, xmax, ymin, ymax of the mesh the plane belongs to."""
    box = mesh_bbox(x, y) if bbox is None else np.asarray(bbox, np.float64)
    pminx, pmaxx, pminy, pmaxy = (float(v) for v in box)
    DDx, DDy = (pmaxx - pminx) * 0.05, (pmaxy - pminy) * 0.05
    pminx, pminy, pmaxx, pmaxy = pminx - DDx, pminy - DDy, pmaxx + DDx, pmaxy + DDy
    coef = 1073741823. / max(pmaxx - pminx, pmaxy - pminy)
    fx, fy = coef * (x - pminx), coef * (y - pminy)
    assert ((fx >= 0) & (fx < 1073741824.) & (fy >= 0) & (fy < 1073741824.)).all()
    return np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64), (coef, pminx, pminy, box)


def _det(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def locate(x, y, tri, px, py, bbox=None):
    """Triangle (or -1) and the three integer area coordinates of every point; points outside the isdefault box are not looked for."""
    ix, iy, (coef, pminx, pminy, box) = int_plane(x, y, bbox)
    n = px.size
    it = np.full(n, -1, np.int64)
    dd = np.zeros((n, 3), np.int64)
    with np.errstate(invalid="ignore"):
        inbox = ~((px < box[0]) | (px > box[1]) | (py < box[2]) | (py > box[3]))
    inbox &= np.isfinite(px) & np.isfinite(py)
    sel = np.flatnonzero(inbox)
    Bx = np.trunc(coef * (px[sel] - pminx)).astype(np.int64); By = np.trunc(coef * (py[sel] - pminy)).astype(np.int64)
    got = np.full(sel.size, -1, np.int64)
    dsel = np.zeros((sel.size, 3), np.int64)
    x0, y0, x1, y1, x2, y2 = ix[tri[:, 0]], iy[tri[:, 0]], ix[tri[:, 1]], iy[tri[:, 1]], ix[tri[:, 2]], iy[tri[:, 2]]
    CH = 256
    for lo in range(0, tri.shape[0], CH):
        s = slice(lo, lo + CH)
        e0 = _det(x1[s, None], y1[s, None], x2[s, None], y2[s, None], Bx[None, :], By[None, :])
        e1 = _det(x2[s, None], y2[s, None], x0[s, None], y0[s, None], Bx[None, :], By[None, :])
        e2 = _det(x0[s, None], y0[s, None], x1[s, None], y1[s, None], Bx[None, :], By[None, :])
        hit = (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & ((e0 + e1 + e2) > 0)
        anyhit = hit.any(0) & (got < 0)
        first = hit.argmax(0)                      # the lowest triangle number of the chunk
        cols = np.flatnonzero(anyhit)
        got[cols] = lo + first[cols]
        dsel[cols, 0] = e0[first[cols], cols]; dsel[cols, 1] = e1[first[cols], cols]; dsel[cols, 2] = e2[first[cols], cols]
    it[sel] = got; dd[sel] = dsel
    return it, dd


def found_flags(it, n_owned=None):
    f = (it >= 0).astype(np.int32)
    if n_owned is not None:
        f[it >= n_owned] = 2
    return f


def move(x, y, tri, UT, px, py, bbox=None, n_owned=None):
    """Drifters::move: UT = [u | v] on the nodes; returns the new positions, found, and (it, dd).  Only drifters in an owned element move."""
    it, dd = locate(x, y, tri, px, py, bbox)
    f = found_flags(it, n_owned)
    nn = x.size
    qx, qy = px.copy(), py.copy()
    m = np.flatnonzero(f == 1)
    det = (dd[m, 0] + dd[m, 1] + dd[m, 2]).astype(np.float64)
    a0, a1, a2 = dd[m, 0].astype(np.float64) / det, dd[m, 1].astype(np.float64) / det, dd[m, 2].astype(np.float64) / det
    i0, i1, i2 = tri[it[m], 0], tri[it[m], 1], tri[it[m], 2]
    du = a0 * UT[i0] + a1 * UT[i1] + a2 * UT[i2]
    dv = a0 * UT[nn + i0] + a1 * UT[nn + i1] + a2 * UT[nn + i2]
    qx[m] = px[m] + du; qy[m] = py[m] + dv
    return qx, qy, f, it, dd


def conc(x, y, tri, UM, conc_el, px, py, bbox=None, n_owned=None):
    """Drifters::updateConc: the mesh displaced by UM = [u | v], a P0 look-up, std::max(0., std::min(1., v)) as the two comparisons."""
    nn = x.size
    it, dd = locate(x + UM[:nn], y + UM[nn:], tri, px, py, bbox)
    v = np.zeros(px.size)
    v[it >= 0] = conc_el[it[it >= 0]]
    lo = np.where(v < 1., v, 1.)
    return np.where(0. < lo, lo, 0.), found_flags(it, n_owned), it, dd


def mask(conc_d, ids, conc_lim, keepers=None):
    """Drifters::maskXY: the indices of the survivors, in order."""
    keep = conc_d > conc_lim
    if keepers is not None:
        keep &= np.isin(ids, np.asarray(keepers))
    return np.flatnonzero(keep)
