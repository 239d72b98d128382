"""Generates tests/golden/means_points.npz with the REAL contrib/bamg (oracle/_ref, built by `python __graft_entry__.py` where the reference is present):
    python tests/golden/make_means_points_golden.py

GridOutput::updateGridMean() on a LOADED grid chained exactly as model/gridoutput.cpp:387-415 chains it -- three InterpFromMeshToMesh2dx calls with isdefault = true
and default 0. (proc mask, elemental variables, nodal variables), rotateVectors per pair, the product with the proc mask, the accumulation, the ice-mask rule --
twice, in two differently displaced meshes (UM1, UM2), then setLSM on the mesh at rest and applyLSM.  Every interpolation is made by the real library.
  ge1, gn1 / ge2, gn2   the grid accumulators after the first / the second updateGridMean, rotation NORTH_EAST (gridLON)
  gn2_theta             the nodal accumulators after both with rotation GRID_THETA (gridTheta); the elemental ones do not depend on the rotation
  lsm                   setLSM;  ge2_lsm, gn2_lsm: after applyLSM
  it1, dd1, it2, dd2    the triangle and the integer area coordinates of every grid point in the two displaced meshes (tests/drifters_ref.locate: what the host
                        build of the per-point body is fed); gx, gy the grid
Mesh: cases.mesh_with_holes("small") -- an outer coast and two islands; the last third of the elements is declared ghost.  Grid: curvilinear, rotated and
stretched, 41 x 53 points reaching 10 % beyond the mesh's box: points outside the box, between box and coast, in an island, in ghost and in owned elements.
Variables: conc, thick (masked), ice_mask; VT_x, VT_y (masked), tau_ax, tau_ay with the pairs (0, 1) and (2, 3).  The seeded accumulator rows hold negative
values, a row of zeros, ice_mask <= 0 and > 0, and one NaN node that a grid point in an owned and one in a ghost element see.

NO TIES: a grid point exactly on an edge or a vertex is the one case in which the reference's own answer depends on its triangle walk.  means_points_case() is
seeded (SEED) so that NO grid point inside the mesh has a zero integer area coordinate, in either displaced mesh or at rest; main() asserts it (zero points are
left out) before it writes the file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
import drifters_ref as R  # noqa: E402
import means_points_ref as P  # noqa: E402

SEED = 7
NU, NV = 41, 53
MISS = -1e14
ELEMENTAL = ("conc", ("thick", True), "ice_mask")
NODAL = ("VT_x", ("VT_y", True), "tau_ax", "tau_ay")
EL_MASK, NOD_MASK, ICE_COL = (0, 1, 0), (0, 1, 0, 0), 2
PAIRS = ((0, 1), (2, 3))
ROTATION_ANGLE = -45. * P.PI / 180.
OUT = os.path.join(HERE, "means_points.npz")


def curvilinear_grid(x, y, nu=NU, nv=NV, reach=1.1, seed=SEED):
    """A rotated, stretched nu x nv grid whose extent is `reach` times the box of (x, y); gridLON in degrees, gridTheta in radians."""
    rng = np.random.default_rng(seed + 1000)
    U, V = np.meshgrid(np.linspace(-1., 1., nu), np.linspace(-1., 1., nv), indexing="ij")
    t = np.deg2rad(20.)
    X = np.cos(t) * U * (1. + 0.10 * V) - np.sin(t) * V * (1. + 0.15 * U * U)
    Y = np.sin(t) * U * (1. - 0.20 * V * V) + np.cos(t) * V * (1. + 0.05 * U)
    X, Y = X / np.abs(X).max(), Y / np.abs(Y).max()
    cx, cy, wx, wy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max()), np.ptp(x), np.ptp(y)
    gx = (cx + 0.5 * reach * wx * X).ravel() + 1e-3 * wx / nu * rng.standard_normal(nu * nv)
    gy = (cy + 0.5 * reach * wy * Y).ravel() + 1e-3 * wy / nv * rng.standard_normal(nu * nv)
    lon = np.degrees(np.arctan2(gx, -gy)) + 45.
    theta = 0.3 * np.sin(2. * U).ravel() + 0.2 * V.ravel() - 0.1
    return np.ascontiguousarray(gx), np.ascontiguousarray(gy), np.ascontiguousarray(lon), np.ascontiguousarray(theta)


def means_points_case():
    """Seeded inputs of the fixture."""
    x, y, tri = cases.mesh_with_holes("small")
    rng = np.random.default_rng(SEED)
    nn, ne = x.size, tri.shape[0]
    n_owned = ne - ne // 3
    xs, ys = x[tri], y[tri]
    area = 0.5 * np.abs((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0]))
    h = float(np.sqrt(2. * area.mean()))
    L = max(np.ptp(x), np.ptp(y))
    UM1 = np.concatenate([0.04 * h * np.sin(3. * x / L) * np.cos(2. * y / L + 0.1), 0.04 * h * np.cos(2. * x / L + 0.7) * np.sin(3. * y / L)])
    UM2 = np.concatenate([-3.0 * UM1[nn:], 2.5 * UM1[:nn]])          # another displaced mesh, a tenth of an element: no triangle flips
    gx, gy, lon, theta = curvilinear_grid(x, y)
    el = rng.normal(0., 1., (ne, len(ELEMENTAL)))
    el[:, ICE_COL] = rng.integers(-1, 3, ne).astype(np.float64)      # ice_mask accumulates counts; <= 0 and > 0, a negative one for the rule's other side
    el[n_owned:] = 0.                                                 # updateMeans never touches a ghost row
    nod = rng.normal(0., 5., (nn, len(NODAL)))
    # a row of zeros and the NaN node: both where grid points look.  The NaN node is a vertex of an owned AND of a ghost element that each hold a grid point
    it1, _ = R.locate(x + UM1[:nn], y + UM1[nn:], tri, gx, gy)
    hit = np.unique(it1[it1 >= 0])
    el[hit[hit < n_owned][0]] = 0.
    seen_owned, seen_ghost = np.unique(tri[hit[hit < n_owned]]), np.unique(tri[hit[hit >= n_owned]])
    both = np.intersect1d(seen_owned, seen_ghost)
    assert both.size, "no node is seen from an owned and from a ghost element: another grid"
    nan_node = int(both[0])
    nod[nan_node] = np.nan
    return dict(x=x, y=y, tri=np.ascontiguousarray(tri), n_owned=n_owned, UM1=UM1, UM2=UM2, gx=gx, gy=gy, lon=lon, theta=theta, el=el, nod=nod, nan_node=nan_node)


def chain(c, interp, rotation="north_east"):
    """updateGridMean twice (UM1, UM2), setLSM, applyLSM with `interp(x, y, tri, data, px, py, nodal)` = InterpFromMeshToMesh2dx(..., true, 0.) -> [n, N_data]."""
    nn = c["x"].size
    cs, sn = P.cos_sin(rotation, ROTATION_ANGLE, c["lon"], c["theta"])
    ge, gn = np.zeros((len(ELEMENTAL), c["gx"].size)), np.zeros((len(NODAL), c["gx"].size))
    out = {}
    for k, UM in ((1, c["UM1"]), (2, c["UM2"])):
        P.update_grid_mean(ge, gn, c["x"] + UM[:nn], c["y"] + UM[nn:], c["tri"], c["n_owned"], c["el"], c["nod"], c["gx"], c["gy"], PAIRS, cs, sn, MISS, ICE_COL,
                           EL_MASK, NOD_MASK, interp)
        out[f"ge{k}"], out[f"gn{k}"] = ge.copy(), gn.copy()
    out["lsm"] = P.set_lsm(c["x"], c["y"], c["tri"], c["gx"], c["gy"], interp)
    out["ge2_lsm"], out["gn2_lsm"] = P.apply_lsm(ge, out["lsm"], MISS), P.apply_lsm(gn, out["lsm"], MISS)
    return out


def real_bamg(x, y, tri, data, px, py, nodal):
    from oracle import pyoracle as O
    data = np.asarray(data, np.float64)
    assert data.shape[0] == (x.size if nodal else tri.shape[0]) and x.size != tri.shape[0]      # (the library tells the two apart by the length)
    return O.bamg_interp_mesh_to_mesh((tri + 1).astype(np.int32).ravel(), x, y, data, px, py, True, 0.)


def ties(c):
    nn = c["x"].size
    return tuple(P.ties(c["x"] + UM[:nn], c["y"] + UM[nn:], c["tri"], c["gx"], c["gy"]) for UM in (c["UM1"], c["UM2"], np.zeros(2 * nn)))


def located(c):
    nn = c["x"].size
    out = {}
    for k, UM in ((1, c["UM1"]), (2, c["UM2"])):
        it, dd = R.locate(c["x"] + UM[:nn], c["y"] + UM[nn:], c["tri"], c["gx"], c["gy"])
        out[f"it{k}"], out[f"dd{k}"] = it.astype(np.int32), dd
    return out


def main():
    c = means_points_case()
    assert ties(c) == (0, 0, 0), ties(c)          # pick another SEED rather than leave a point out
    g = chain(c, real_bamg)
    g["gn2_theta"] = chain(c, real_bamg, "grid_theta")["gn2"]
    loc = located(c)
    box = R.mesh_bbox(c["x"] + c["UM1"][:c["x"].size], c["y"] + c["UM1"][c["x"].size:])
    outside = (c["gx"] < box[0]) | (c["gx"] > box[1]) | (c["gy"] < box[2]) | (c["gy"] > box[3])
    it = loc["it1"]
    assert outside.any() and ((it < 0) & ~outside).any() and (it >= c["n_owned"]).any() and ((it >= 0) & (it < c["n_owned"])).any()
    assert np.isnan(g["gn1"]).any() and (g["lsm"] == 0).any() and (g["lsm"] == 1).any()
    np.savez_compressed(OUT, gx=c["gx"], gy=c["gy"], **loc, **g)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in g.items()}, "outside the box:", int(outside.sum()), "in no triangle:", int((it < 0).sum()),
          "ghost:", int((it >= c["n_owned"]).sum()), "NaN:", int(np.isnan(g["gn2"]).sum()))


if __name__ == "__main__":
    main()
