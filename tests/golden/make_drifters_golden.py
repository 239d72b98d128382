"""Generates tests/golden/drifters.npz with the REAL contrib/bamg (oracle/_ref, built by `python __graft_entry__.py` where the reference is present):
    python tests/golden/make_drifters_golden.py

The three statements of checkUpdateDrifters() (FE.cpp:8403-8437) chained as model/drifters.cpp chains them, every interpolation made by the real
InterpFromMeshToMesh2dx with isdefault = true and default 0.:
  x1, y1     the drifters after Drifters::move (M_UT interleaved as drifters.cpp:483-487, interpolated in the undisplaced mesh, added)
  conc       Drifters::updateConc at the moved positions in the mesh displaced by M_UM, clamped to [0, 1]
  keep_all   the survivors (indices into the 5 003) of maskXY with conc_lim = 0.15 and every id
  keep_third of those, the survivors of maskXY with the keepers list KEEPERS (every third id)
Mesh: cases.mesh_with_holes("small") -- an outer coast and two islands.  Drifters: 5 003 over the mesh's bounding box grown by 10 %: some start outside
the box, some in an island, some between coast and box.  M_UT is a smooth field a few element sizes large (some drifters leave the mesh), M_UM a smooth
field a fraction of an element large (no triangle flips), M_conc seeded random per element in [-0.1, 1.1] (the clamp works on both sides).

NO TIES: a drifter exactly on an edge or a vertex of the mesh is the one case in which the reference's own answer depends on the history of its triangle
walk.  drifters_case() is seeded (SEED) so that NO drifter inside the mesh has a zero integer area coordinate, neither at its start in the undisplaced
mesh nor after the move in the displaced one; main() asserts it (zero drifters are left out on that ground) before it writes the file."""
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

SEED = 20
N_DRIFTERS = 5003
CONC_LIM = 0.15
OUT = os.path.join(HERE, "drifters.npz")


def drifters_case():
    """Seeded inputs of the fixture: x, y, tri (0-based) of the mesh, UT, UM ([u | v]), conc per element, the drifters px, py, ids, the keepers list."""
    x, y, tri = cases.mesh_with_holes("small")
    rng = np.random.default_rng(SEED)
    nn, ne = x.size, tri.shape[0]
    xs, ys = x[tri], y[tri]
    area = 0.5 * np.abs((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0]))
    h = float(np.sqrt(2. * area.mean()))                     # an element size
    L = max(np.ptp(x), np.ptp(y))
    UT = np.concatenate([3.0 * h * np.sin(5. * y / L + 0.3) * np.cos(3. * x / L), 2.5 * h * np.cos(4. * x / L - 0.2) + 0.5 * h * np.sin(7. * y / L)])
    UM = np.concatenate([0.04 * h * np.sin(3. * x / L) * np.cos(2. * y / L + 0.1), 0.04 * h * np.cos(2. * x / L + 0.7) * np.sin(3. * y / L)])
    conc = rng.uniform(-0.1, 1.1, ne)
    cx, cy, wx, wy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max()), np.ptp(x), np.ptp(y)
    px = cx + 1.1 * wx * (rng.random(N_DRIFTERS) - 0.5)
    py = cy + 1.1 * wy * (rng.random(N_DRIFTERS) - 0.5)
    ids = rng.permutation(3 * N_DRIFTERS)[:N_DRIFTERS].astype(np.int32)
    keepers = np.ascontiguousarray(ids[::3])
    assert nn == UT.size // 2
    return dict(x=x, y=y, tri=tri, UT=UT, UM=UM, conc=conc, px=px, py=py, ids=ids, keepers=keepers)


def chain(c, interp):
    """The three statements with `interp(x, y, tri, data, px, py)` = InterpFromMeshToMesh2dx(..., isdefault = true, 0.) returning [n, N_data]."""
    nn = c["x"].size
    inter = np.stack([c["UT"][:nn], c["UT"][nn:]], 1)                                   # drifters.cpp:483-487
    d = interp(c["x"], c["y"], c["tri"], inter, c["px"], c["py"])
    x1, y1 = c["px"] + d[:, 0], c["py"] + d[:, 1]                                      # drifters.cpp:499-503
    v = interp(c["x"] + c["UM"][:nn], c["y"] + c["UM"][nn:], c["tri"], c["conc"], x1, y1)[:, 0]
    lo = np.where(v < 1., v, 1.)
    cd = np.where(0. < lo, lo, 0.)                                                     # drifters.cpp:538-539
    keep_all = R.mask(cd, c["ids"], CONC_LIM)
    keep_third = keep_all[R.mask(cd[keep_all], c["ids"][keep_all], CONC_LIM, c["keepers"])]
    return dict(x1=x1, y1=y1, conc=cd, keep_all=keep_all.astype(np.int32), keep_third=keep_third.astype(np.int32))


def real_bamg_chain(c):
    from oracle import pyoracle as O

    def interp(x, y, tri, data, px, py):
        return O.bamg_interp_mesh_to_mesh((tri + 1).astype(np.int32).ravel(), x, y, data, px, py, True, 0.)
    return chain(c, interp)


def ties(c):
    """How many drifters inside the mesh have a zero integer area coordinate: at the start in the undisplaced mesh, after the move in the displaced one."""
    nn = c["x"].size
    x1, y1, f, it, dd = R.move(c["x"], c["y"], c["tri"], c["UT"], c["px"], c["py"])
    t0 = int(((dd == 0).any(1) & (it >= 0)).sum())
    it2, dd2 = R.locate(c["x"] + c["UM"][:nn], c["y"] + c["UM"][nn:], c["tri"], x1, y1)
    return t0, int(((dd2 == 0).any(1) & (it2 >= 0)).sum())


def main():
    c = drifters_case()
    assert ties(c) == (0, 0), ties(c)          # pick another SEED rather than leave a drifter out
    g = real_bamg_chain(c)
    np.savez_compressed(OUT, px=c["px"], py=c["py"], ids=c["ids"], **g)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
