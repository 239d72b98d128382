"""Generates tests/golden/means_regular.npz with the REAL contrib/bamg (oracle/_ref, built by `python __graft_entry__.py` where the reference is present):
    python tests/golden/make_means_regular_golden.py

GridOutput::updateGridMean() on the REGULAR grid chained exactly as model/gridoutput.cpp:387-415 chains it -- three InterpFromMeshToGridx calls with default 0.
(proc mask, elemental variables, nodal variables), rotateVectors per pair, the product with the proc mask, the transposed accumulation, the ice-mask rule -- twice,
in two differently displaced meshes (UM1, UM2), with setLSM on the mesh at rest and applyLSM at the end.  Every interpolation is made by the real library through
oracle.pyoracle.bamg_interp_mesh_to_grid.
  lsm                   setLSM (before the updates, as initMoorings does)
  ge1, gn1 / ge2, gn2   the grid accumulators after the first / the second updateGridMean, rotation NONE
  gn2_ne                the nodal accumulators after both with rotation NORTH_EAST (the elemental ones do not depend on the rotation)
  ge2_lsm, gn2_ne_lsm   after applyLSM
  hit0, hit1, hit2      the element each grid point ended up with at rest / in the two displaced meshes (an interpolation of the element numbers), grid order
Mesh: cases.mesh_with_holes("small") -- an outer coast and two islands; the last third of the elements is declared ghost; SNAP of its nodes are moved ONTO the
grid's lattice (whole rows of neighbours, so lattice points also lie on shared edges), where UM1 is zero: those grid points are held by several triangles and the
highest-number rule decides them.  Grid: 19 x 41 points (ncols != nrows) that cover a part of the mesh around the smaller island and reach beyond the mesh's box.
Variables: conc, thick (masked), ice_mask; VT_x, VT_y (masked), tau_ax, tau_ay with the pairs (0, 1) and (2, 3)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
import means_regular_ref as Q  # noqa: E402

SEED = 11
MISS = -1e14
NCOLS, NROWS, SPACING = 19, 41, 45e3
XMIN, YMAX = -1.26e6, 2.43e6
GRID = dict(xmin=XMIN, ymax=YMAX, spacing=SPACING, ncols=NCOLS, nrows=NROWS)
ELEMENTAL = ("conc", ("thick", True), "ice_mask")
NODAL = ("VT_x", ("VT_y", True), "tau_ax", "tau_ay")
EL_MASK, NOD_MASK, ICE_COL = (0, 1, 0), (0, 1, 0, 0), 2
PAIRS = ((0, 1), (2, 3))
ROTATION_ANGLE = -45. * Q.PI / 180.
OUT = os.path.join(HERE, "means_regular.npz")


def grid_lon(g=GRID):
    """gridLON in degrees as initRegularGrid fills it: entry i + ncols * j is the longitude of the point (i, j) (a made-up projection: any numbers do)."""
    gx, gy = Q.grid_points(g)
    return np.degrees(np.arctan2(gx, -gy)) + 45.


def means_regular_case():
    """Seeded inputs of the fixture."""
    x, y, tri = cases.mesh_with_holes("small")
    x, y = x.copy(), y.copy()
    rng = np.random.default_rng(SEED)
    nn, ne = x.size, tri.shape[0]
    n_owned = ne - ne // 3
    x_grid, y_grid = Q.grid_axes(XMIN, YMAX, SPACING, SPACING, NCOLS, NROWS)
    # nodes onto the lattice: every node within a fifth of the spacing of a lattice point moves there (far less than an element: no triangle flips)
    ix, iy = np.rint((x - x_grid[0]) / SPACING).astype(int), np.rint((y - y_grid[0]) / SPACING).astype(int)
    near = (ix >= 0) & (ix < NCOLS) & (iy >= 0) & (iy < NROWS)
    lx, ly = x_grid[np.clip(ix, 0, NCOLS - 1)], y_grid[np.clip(iy, 0, NROWS - 1)]
    snap = near & (np.hypot(x - lx, y - ly) < 0.2 * SPACING)
    # ... and a whole row of neighbours: the nodes of one mesh row near the grid row through the first snapped node take that row's y (lattice points on shared edges)
    row = near & (np.abs(y - ly) < 0.25 * SPACING) & (iy == iy[np.flatnonzero(snap)[0]])
    x[snap], y[snap] = lx[snap], ly[snap]
    y[row] = ly[row]
    snap = snap | row
    xs, ys = x[tri], y[tri]
    jac = (xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0])
    assert (jac > 0).all(), "a moved node flipped a triangle"
    h = float(np.sqrt(np.abs(jac).mean()))
    L = max(np.ptp(x), np.ptp(y))
    UM1 = np.concatenate([0.04 * h * np.sin(3. * x / L) * np.cos(2. * y / L + 0.1), 0.04 * h * np.cos(2. * x / L + 0.7) * np.sin(3. * y / L)])
    UM1[:nn][snap] = 0.; UM1[nn:][snap] = 0.                        # the lattice nodes stay on the lattice in the first displaced mesh
    UM2 = np.concatenate([-3.0 * UM1[nn:], 2.5 * UM1[:nn]]) + 0.1 * h  # another displaced mesh, a tenth of an element: no triangle flips, points change triangles
    el = rng.normal(0., 1., (ne, len(ELEMENTAL)))
    el[:, ICE_COL] = rng.integers(-1, 3, ne).astype(np.float64)      # ice_mask accumulates counts; <= 0 and > 0, a negative one for the rule's other side
    el[n_owned:] = 0.                                                 # updateMeans never touches a ghost row
    nod = rng.normal(0., 5., (nn, len(NODAL)))
    hit1 = Q.find_winners(x + UM1[:nn], y + UM1[nn:], tri, GRID)
    won = np.unique(hit1[hit1 >= 0])
    owned, ghost = won[won < n_owned], won[won >= n_owned]
    assert owned.size and ghost.size, "the grid sees no owned or no ghost element: another grid"
    el[owned[0]] = 0.                                                 # a row of zeros
    el[owned[1], 0] = np.nan                                          # a NaN elemental value
    both = np.intersect1d(np.unique(tri[owned]), np.unique(tri[ghost]))
    assert both.size, "no node is seen from an owned and from a ghost element: another grid"
    nan_node = int(both[0])
    nod[nan_node] = np.nan                                            # the all-NaN nodal row
    # tau_ax == miss_val on a patch of nodes: a1 * m + a2 * m + a3 * m is m itself at some of the points inside (rotateVectors skips those)
    centre = tri[owned[owned.size // 2], 0]
    patch = np.hypot(x - x[centre], y - y[centre]) < 3. * h
    patch[nan_node] = False
    nod[patch, 2] = MISS
    return dict(x=x, y=y, tri=np.ascontiguousarray(tri), n_owned=n_owned, UM1=UM1, UM2=UM2, el=el, nod=nod, nan_node=nan_node, snap=np.flatnonzero(snap),
                patch=np.flatnonzero(patch), lon=grid_lon())


def chain(c, interp, rotation="none"):
    """setLSM, updateGridMean twice (UM1, UM2), applyLSM with `interp` = InterpFromMeshToGridx."""
    nn, G = c["x"].size, NCOLS * NROWS
    cs, sn = Q.cos_sin(rotation, ROTATION_ANGLE, c["lon"])
    ge, gn = np.zeros((len(ELEMENTAL), G)), np.zeros((len(NODAL), G))
    out = {"lsm": Q.set_lsm(c["x"], c["y"], c["tri"], GRID, interp)}
    for k, UM in ((1, c["UM1"]), (2, c["UM2"])):
        Q.update_grid_mean(ge, gn, c["x"] + UM[:nn], c["y"] + UM[nn:], c["tri"], c["n_owned"], c["el"], c["nod"], GRID, PAIRS, cs, sn, MISS, ICE_COL, EL_MASK, NOD_MASK, interp)
        out[f"ge{k}"], out[f"gn{k}"] = ge.copy(), gn.copy()
    out["ge2_lsm"], out["gn2_lsm"] = Q.apply_lsm(ge, out["lsm"], MISS), Q.apply_lsm(gn, out["lsm"], MISS)
    return out


def winners(c, interp):
    nn = c["x"].size
    return {f"hit{k}": Q.find_winners(c["x"] + UM[:nn], c["y"] + UM[nn:], c["tri"], GRID, interp) for k, UM in ((0, np.zeros(2 * nn)), (1, c["UM1"]), (2, c["UM2"]))}


def real_bamg(*args):
    from oracle import pyoracle as O
    return O.bamg_interp_mesh_to_grid(*args)


def main():
    c = means_regular_case()
    g = chain(c, real_bamg)
    ne = chain(c, real_bamg, "north_east")
    z = dict(lsm=g["lsm"], ge1=g["ge1"], gn1=g["gn1"], ge2=g["ge2"], gn2=g["gn2"], gn2_ne=ne["gn2"], ge2_lsm=g["ge2_lsm"], gn2_ne_lsm=ne["gn2_lsm"], **winners(c, real_bamg))
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in z.items()})


if __name__ == "__main__":
    main()
