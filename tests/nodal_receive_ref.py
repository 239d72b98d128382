"""The coupler's receive of NODAL fields restated line by line (numpy; no device, no library):

    receiveCouplingData    model/externaldata.cpp:498-509     t = field[reduced[i]]; t *= a; t += b
    transformData          externaldata.cpp:944-1288          the east/north branch (tests/nodal_forcing_ref.transform: section 6l's host body), then
                                                              rotation_angle != 0. (:1246-1261) else gridded_rotation_angle (:1263-1281)
    _apply                 contrib/bamg/src/InterpFromMeshToMesh2dx_apply.cpp:57-59     a0*d[v0] + a1*d[v1] + a2*d[v2], left to right
    ExternalData::get      externaldata.cpp:434, 438          factor*x + bias ("coupled": nb_forcing_step == 1)

and the seeded inputs of tests/golden/nodal_receive.npz (made by tests/golden/make_nodal_receive_golden.py with the REAL bamg).  The three weights and vertices of
a target are read OUT OF THE FIXTURE (weights_from_dense): the real library's interpolation of the identity matrix returns each weight exactly, the triangle that
holds the non-zero ones gives the order of the three products.  `mistake` plants one wrong statement at a time (tests/test_nodal_receive_ref.py: each changes a bit)."""
import math
import os

import numpy as np

import cases
import drifters_ref as D
import nodal_forcing_ref as NF

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "nodal_receive.npz")
SEED = 11
NU, NV = 7, 9                      # the exchange grid: G = 63 points
CASES = ("full", "strip", "notch")
MISTAKES = ("a_b_swapped", "rotation_sign", "reduced_ignored", "weights_permuted", "factor_before_sum", "rotate_after_gather")


def exchange_grid(seed=SEED):
    """A curvilinear NU x NV grid whose four sides bulge OUTWARDS (so that the wet set's boundary is strictly convex unless it is notched), rotated by 20 degrees:
    x, y [G] in metres, point (i, j) at i*NV + j; theta [G] radians (grid.gridTheta); lat, lon [G] degrees."""
    rng = np.random.default_rng(seed)
    U, V = np.meshgrid(np.linspace(-1., 1., NU), np.linspace(-1., 1., NV), indexing="ij")
    X0 = U * (1. + 0.08 * (1. - V * V))
    Y0 = V * (1. + 0.08 * (1. - U * U))
    t = np.deg2rad(20.)
    x = 4.0e5 * (np.cos(t) * X0 - np.sin(t) * Y0).ravel() + 2.0e4
    y = 5.0e5 * (np.sin(t) * X0 + np.cos(t) * Y0).ravel() - 1.0e4
    x = x + 50. * rng.standard_normal(x.size)
    y = y + 50. * rng.standard_normal(y.size)
    theta = (0.3 * np.sin(2. * U) + 0.2 * V - 0.1).ravel()
    lat = (78. + 8. * V - 2. * U * U).ravel()
    lon = (30. + 150. * U + 20. * V).ravel()
    return np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(theta), np.ascontiguousarray(lat), np.ascontiguousarray(lon)


def wet_mask(name):
    """[NU, NV] True = wet.  full: no mask; strip: the column j = 0 masked (a convex wet set, reduced a strict subset that does not start at 0);
    notch: two points in the middle of the side j = 0 masked (the completion of the wet set has fill triangles)."""
    m = np.ones((NU, NV), bool)
    if name == "strip":
        m[:, 0] = False
    elif name == "notch":
        m[3, 0] = m[3, 1] = False
    elif name != "full":
        raise KeyError(name)
    return m


def source(name, seed=SEED):
    """The reduced source of a case: reduced [R] (grid.reduced_nodes_ind), the wet nodes' x, y, theta, lat, lon [R] and tri [nels, 3] (0-based, counter-clockwise:
    the two triangles of every grid cell whose four corners are wet)."""
    x, y, theta, lat, lon = exchange_grid(seed)
    m = wet_mask(name)
    reduced = np.flatnonzero(m.ravel()).astype(np.int32)
    new = np.full(NU * NV, -1, np.int64)
    new[reduced] = np.arange(reduced.size)
    tri = []
    for i in range(NU - 1):
        for j in range(NV - 1):
            c = [i * NV + j, (i + 1) * NV + j, (i + 1) * NV + j + 1, i * NV + j + 1]
            if m.ravel()[c].all():
                tri += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    tri = np.ascontiguousarray(new[np.array(tri)], np.int32)
    assert (tri >= 0).all() and np.unique(tri).size == reduced.size
    xs, ys = x[reduced][tri], y[reduced][tri]
    assert (((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0])) > 0).all()
    return dict(G=NU * NV, reduced=reduced, x=x[reduced].copy(), y=y[reduced].copy(), theta=theta[reduced].copy(), lat=lat[reduced].copy(), lon=lon[reduced].copy(),
                tri=tri)


def unmappable_source(seed=SEED):
    """A source the convex completion REFUSES (x, y, tri 0-based, the reason it gives): two copies of the full exchange grid joined corner to corner by two
    DISTINCT nodes on one point -- a duplicated node nobody merged.  The pocket construction sees two outer boundary loops, the general one two boundary vertices
    on one integer point; InterpFromMeshToMesh2dx has no meaning there, and a node map made of it would hold the nearest-boundary-edge stand-in's weights."""
    src = source("full", seed)
    x, y, tri = src["x"], src["y"], src["tri"]
    hi, lo = int(np.argmax(x + y)), int(np.argmin(x + y))
    x2, y2 = np.concatenate([x, x + (x[hi] - x[lo])]), np.concatenate([y, y + (y[hi] - y[lo])])
    x2[x.size + lo], y2[x.size + lo] = x2[hi], y2[hi]      # (the shift's rounding may leave the two a last bit apart: the same point, exactly)
    return np.ascontiguousarray(x2), np.ascontiguousarray(y2), np.ascontiguousarray(np.concatenate([tri, tri + x.size]), np.int32), "two boundary vertices share one integer point"


def targets(src):
    """The nodes of cases.mesh_with_holes("small"), scaled to reach 10 % beyond the box of the source: targets inside, beyond an edge, in the cone of a hull vertex."""
    tx, ty, _ = cases.mesh_with_holes("small")
    cx, cy = 0.5 * (src["x"].min() + src["x"].max()), 0.5 * (src["y"].min() + src["y"].max())
    px = cx + 1.1 * np.ptp(src["x"]) * (tx - 0.5 * (tx.min() + tx.max())) / np.ptp(tx)
    py = cy + 1.1 * np.ptp(src["y"]) * (ty - 0.5 * (ty.min() + ty.max())) / np.ptp(ty)
    return np.ascontiguousarray(px), np.ascontiguousarray(py)


def ties(src, px, py):
    """Targets inside the source with a zero integer area coordinate: the reference's answer there depends on its walk."""
    it, dd = D.locate(src["x"], src["y"], src["tri"], px, py)
    return int(((dd == 0).any(1) & (it >= 0)).sum())


def hull(x, y):
    """The convex hull of the points, counter-clockwise (Andrew's chain)."""
    pts = sorted(zip(x.tolist(), y.tolist()))

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lo, up = half(pts), half(reversed(pts))
    return np.array(lo[:-1] + up[:-1])


def in_fill(src, px, py):
    """Targets in no triangle of the source but strictly inside its convex hull: where InterpFromMeshToMesh2dx_weights throws."""
    it, _ = D.locate(src["x"], src["y"], src["tri"], px, py)
    h = hull(src["x"], src["y"])
    a, b = h, np.roll(h, -1, axis=0)
    inside = np.ones(px.size, bool)
    for (ax, ay), (bx, by) in zip(a, b):
        inside &= (bx - ax) * (py - ay) - (by - ay) * (px - ax) > 0
    return np.flatnonzero((it < 0) & inside)


def awkward_data(src, seed=SEED):
    """[R, 2] source data: negative values, a row of zeros, one NaN source node two rows inside the wet set (no triangle behind a hull edge holds it, so the walk-
    dependent choice of CloseBoundaryEdge's vertex outcome never meets it)."""
    rng = np.random.default_rng(seed + 1)
    d = rng.normal(-1., 3., (src["reduced"].size, 2))
    full = np.full(NU * NV, -1, np.int64)
    full[src["reduced"]] = np.arange(src["reduced"].size)
    d[full[2 * NV + 5]] = 0.
    d[full[3 * NV + 4]] = np.nan
    return d


def weights_from_dense(W, tri):
    """(v [N, 3] int32, a [N, 3]) out of the real library's interpolation W [N, R] of the identity matrix: the triangle of `tri` that holds every non-zero weight
    of the target, its vertex order, W's entries.  (One non-zero weight -- CloseBoundaryEdge's vertex outcome -- is met by several triangles: the first is taken.)"""
    N = W.shape[0]
    v, a = np.zeros((N, 3), np.int32), np.zeros((N, 3))
    sets = [set(t) for t in tri.tolist()]
    for i in range(N):
        nz = set(np.flatnonzero(W[i]).tolist())
        assert 1 <= len(nz) <= 3, (i, nz)
        k = next(k for k, s in enumerate(sets) if nz <= s)
        v[i] = tri[k]
        a[i] = W[i, tri[k]]
    return v, a


def dense(v, a, R):
    """[N, R] from the six rows (the inverse of weights_from_dense)"""
    W = np.zeros((v.shape[0], R))
    for k in range(3):
        W[np.arange(v.shape[0]), v[:, k]] += a[:, k]
    return W


def apply(v, a, d):
    """_apply.cpp:57-59 on d [R] -> [N]"""
    with np.errstate(invalid="ignore"):
        return a[:, 0] * d[v[:, 0]] + a[:, 1] * d[v[:, 1]] + a[:, 2] * d[v[:, 2]]


def cos_sin_theta(rotation, theta):
    """externaldata.cpp:1272-1273 with the C library's cos / sin"""
    c = np.array([NF._libm.cos(rotation - float(t)) for t in theta])
    s = np.array([NF._libm.sin(rotation - float(t)) for t in theta])
    return c, s


def loaded_data(fields, reduced, a, b, pairs=(), rotate=None, east_west=None, details=None, mistake=None):
    """receiveCouplingData + transformData: [n_var, R].  fields [n_var, G]; pairs = [(j0, j1)]; rotate = None or (c, s), scalars or [R] rows; east_west = None or
    dict(lat, lon [R], forward(lat, lon) -> (x, y))."""
    fields = np.asarray(fields, np.float64)
    n = fields.shape[0]
    a, b = np.broadcast_to(np.asarray(a, np.float64), (n,)), np.broadcast_to(np.asarray(b, np.float64), (n,))
    if mistake == "a_b_swapped":
        a, b = b, a
    idx = np.arange(reduced.size) if mistake == "reduced_ignored" else reduced
    out = np.empty((n, reduced.size))
    for v in range(n):
        t = fields[v][idx].copy()
        t *= a[v]
        t += b[v]
        out[v] = t
    for k, (j0, j1) in enumerate(pairs):
        if east_west is not None:
            cell = np.stack([out[j0], out[j1]], axis=1)[None]          # [1, R, 2]: one row of R points, lat / lon per point
            det = {} if details is not None else None
            cell = NF.transform(cell, east_west["lat"], east_west["lon"], [0.], [(0, 1, True)], east_west["forward"], per_point=True, details=det)
            out[j0], out[j1] = cell[0, :, 0], cell[0, :, 1]
            if details is not None:
                details[k] = det[0]
        if rotate is not None:
            out[j0], out[j1] = rotated(out[j0], out[j1], *rotate, mistake)
    return out


def rotated(t0, t1, c, s, mistake=None):
    if mistake == "rotation_sign":
        s = -s
    with np.errstate(invalid="ignore"):
        return c * t0 + s * t1, -s * t0 + c * t1


def receive(fields, reduced, a, b, v, w, pairs=(), rotate=None, east_west=None, factor=None, bias=None, mistake=None):
    """The whole chain: [n_var, N].  factor = None: interpolated_data as it is (raw); else ExternalData::get's factor*x + bias."""
    late = mistake == "rotate_after_gather"
    d = loaded_data(fields, reduced, a, b, pairs, None if late else rotate, east_west, mistake=mistake)
    if mistake == "weights_permuted":
        w = np.roll(w, 1, axis=1)
    n = d.shape[0]
    with np.errstate(invalid="ignore"):
        if mistake == "factor_before_sum" and factor is not None:
            f = np.broadcast_to(np.asarray(factor, np.float64), (n,))
            out = np.stack([(f[k] * w[:, 0]) * d[k][v[:, 0]] + (f[k] * w[:, 1]) * d[k][v[:, 1]] + (f[k] * w[:, 2]) * d[k][v[:, 2]] for k in range(n)])
        else:
            out = np.stack([apply(v, w, d[k]) for k in range(n)])
        if late and rotate is not None:
            c, s = rotate
            if np.ndim(c):      # a per-point angle has no meaning at a target: the mistake interpolates it
                c, s = apply(v, w, c), apply(v, w, s)
            for j0, j1 in pairs:
                out[j0], out[j1] = rotated(out[j0], out[j1], c, s)
        if factor is not None:
            f, bi = np.broadcast_to(np.asarray(factor, np.float64), (n,)), np.broadcast_to(np.asarray(bias, np.float64), (n,))
            if mistake != "factor_before_sum":
                out = np.stack([f[k] * out[k] + bi[k] for k in range(n)])
            else:
                out = np.stack([out[k] + bi[k] for k in range(n)])
    return out


def fields_case(G, n_var=3, seed=SEED):
    """Seeded [n_var, G] fields as a coupler delivers them: land points hold a fill value the reduced index must skip."""
    rng = np.random.default_rng(seed + 10 * n_var)
    f = rng.normal(0.1, 0.5, (n_var, G))
    f[:, ::NV] = 1e20        # the column j = 0, land in the strip case
    return f


def synthetic_case(R, N, n_var, seed=SEED):
    """A map nobody located: R reduced points out of G = R + 7, N targets with random vertices below R and random area coordinates (one of them negative now and
    then, as beyond a hull edge never happens but an imported map may hold) -- what the launch edges of the source and the gather kernel need, at any R and N."""
    rng = np.random.default_rng(seed + 1000 * R + N)
    G = R + 7
    reduced = np.sort(rng.choice(G, R, replace=False)).astype(np.int32)
    v = rng.integers(0, R, (N, 3)).astype(np.int32)
    w = rng.uniform(-0.1, 1., (N, 3))
    w /= w.sum(1)[:, None]
    return dict(G=G, reduced=reduced, theta=rng.uniform(-1., 1., R), lat=rng.uniform(60., 89., R), lon=rng.uniform(-180., 360., R), v=v, w=w,
                fields=rng.normal(0.1, 0.5, (n_var, G)))


def equal(a, b):
    """The same bits, NaN by position"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


UNIFORM_ANGLE = 0.4
MAP_ROTATION = -45. * NF.PI / 180.      # mapNextsim->rotation*PI/180.


def uniform_rotation():
    return math.cos(-UNIFORM_ANGLE), math.sin(-UNIFORM_ANGLE)
