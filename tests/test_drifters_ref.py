"""The drifter fixture (tests/golden/drifters.npz, made by the REAL contrib/bamg) against the numpy restatement the GPU tests compare with
(tests/drifters_ref.py): Drifters::move, updateConc and maskXY (model/drifters.cpp:468-579), bit for bit at every stage."""
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle as O

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import drifters_ref as R  # noqa: E402
import make_drifters_golden as G  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "drifters.npz")


@pytest.fixture(scope="module")
def case():
    return G.drifters_case()


def _ref_interp(x, y, tri, data, px, py):
    """InterpFromMeshToMesh2dx(isdefault = true, 0.) from the restatement: P1 for nodal data [Nn, 2], P0 for element data [Ne]."""
    if data.ndim == 2:
        qx, qy, f, it, dd = R.move(x, y, tri, np.concatenate([data[:, 0], data[:, 1]]), px, py)
        return np.stack([qx - px, qy - py], 1), (qx, qy)
    it, dd = R.locate(x, y, tri, px, py)
    v = np.zeros(px.size)
    v[it >= 0] = data[it[it >= 0]]
    return v[:, None], None


def test_restatement_equals_the_fixture_bit_for_bit(case):
    c, z = case, np.load(GOLD)
    assert np.array_equal(z["px"], c["px"]) and np.array_equal(z["py"], c["py"]) and np.array_equal(z["ids"], c["ids"])
    assert G.ties(c) == (0, 0)      # no drifter of the fixture sits on an edge or a vertex: the reference's answer is unique
    x1, y1, f, it, dd = R.move(c["x"], c["y"], c["tri"], c["UT"], c["px"], c["py"])
    assert np.array_equal(x1, z["x1"]) and np.array_equal(y1, z["y1"])
    cd, f2, it2, dd2 = R.conc(c["x"], c["y"], c["tri"], c["UM"], c["conc"], x1, y1)
    assert np.array_equal(cd, z["conc"])
    keep_all = R.mask(cd, c["ids"], G.CONC_LIM)
    assert np.array_equal(keep_all, z["keep_all"])
    keep_third = keep_all[R.mask(cd[keep_all], c["ids"][keep_all], G.CONC_LIM, c["keepers"])]
    assert np.array_equal(keep_third, z["keep_third"])
    # the fixture exercises what it was built for: drifters outside the box, in an island or beyond the coast, leaving the mesh, both sides of the clamp
    box = R.mesh_bbox(c["x"], c["y"])
    outside = (c["px"] < box[0]) | (c["px"] > box[1]) | (c["py"] < box[2]) | (c["py"] > box[3])
    assert outside.sum() > 100 and ((f == 0) & ~outside).sum() > 100 and ((f == 1) & (f2 == 0)).sum() > 50
    raw = np.where(it2 >= 0, c["conc"][np.maximum(it2, 0)], 0.)
    assert (raw < 0).sum() > 50 and (raw > 1).sum() > 50 and 0 < keep_third.size < keep_all.size < (f2 == 1).sum()


@pytest.mark.skipif(O.bamg_shim() is None, reason="oracle/_ref (real contrib/bamg) not built here")
def test_real_bamg_reproduces_the_committed_fixture(case):
    z = np.load(GOLD)
    g = G.real_bamg_chain(case)
    for k in ("x1", "y1", "conc", "keep_all", "keep_third"):
        assert np.array_equal(g[k], z[k]), k


def test_three_drifters_in_one_triangle_by_hand():
    """One triangle whose integer plane can be written down: box 0..1000 x 0..500 -> pmin = (-50, -25), coef = (2^30 - 1) / 1100."""
    x = np.array([0., 1000., 0.]); y = np.array([0., 0., 500.]); tri = np.array([[0, 1, 2]], np.int32)
    UT = np.array([1., 2., 4., 10., 20., 40.])          # u = 1, 2, 4 and v = 10, 20, 40 on the three vertices
    px = np.array([250., 500., 100.]); py = np.array([125., 100., 300.])
    coef = 1073741823. / 1100.
    ix = [int(coef * (v + 50.)) for v in x]; iy = [int(coef * (v + 25.)) for v in y]
    want_x, want_y = [], []
    for p, q in zip(px, py):
        B = (int(coef * (p + 50.)), int(coef * (q + 25.)))
        det = lambda a, b, c: (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])  # noqa: E731
        V = list(zip(ix, iy))
        dd = [det(V[1], V[2], B), det(V[2], V[0], B), det(V[0], V[1], B)]
        assert min(dd) > 0
        a = [float(d) / float(sum(dd)) for d in dd]
        want_x.append(p + (a[0] * 1. + a[1] * 2. + a[2] * 4.)); want_y.append(q + (a[0] * 10. + a[1] * 20. + a[2] * 40.))
    qx, qy, f, it, dd = R.move(x, y, tri, UT, px, py)
    assert np.array_equal(qx, np.array(want_x)) and np.array_equal(qy, np.array(want_y)) and f.tolist() == [1, 1, 1]
    # the area coordinates are those of the real plane to the truncation of 2^-30 of the box: (0.5, 0.25, 0.25) at (250, 125) -> du = 1/2 + 2/4 + 4/4 = 2, dv = 20
    assert abs(qx[0] - 252.) < 1e-6 and abs(qy[0] - 145.) < 1e-5
    cd, f2, _, _ = R.conc(x, y, tri, np.zeros(6), np.array([1.7]), px, py)
    assert cd.tolist() == [1., 1., 1.]
    cd, _, _, _ = R.conc(x, y, tri, np.zeros(6), np.array([np.nan]), px, py)
    assert cd.tolist() == [1., 1., 1.]                   # std::max(0., std::min(1., NaN)) is 1
    cd, f2, _, _ = R.conc(x, y, tri, np.zeros(6), np.array([-0.2]), np.array([250., 900.]), np.array([125., 400.]))
    assert cd.tolist() == [0., 0.] and f2.tolist() == [1, 0]
    assert R.mask(np.array([0.2, 0.1, 0.9, 0.15]), np.array([7, 8, 9, 10]), 0.15).tolist() == [0, 2]
    assert R.mask(np.array([0.2, 0.1, 0.9, 0.15]), np.array([7, 8, 9, 10]), 0.15, [9, 8]).tolist() == [2]
