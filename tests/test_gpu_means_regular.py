"""The Moorings means on the REGULAR grid on the device (nxs_dyn_means_regular_*): GridOutput::updateGridMean through the M_is_regular_grid branch, setProcMask,
rotateVectors, setLSM / applyLSM, resetGridMean (model/gridoutput.cpp:360-415, 486-538, 558-651) and InterpFromMeshToGridx on the handle's own accumulators, against
the fixture the real contrib/bamg wrote (tests/golden/means_regular.npz), the restatement tests/means_regular_ref.py and the route through the host,
nxs_dyn_means_to_grid.  Bit for bit: there is no tolerance anywhere in this feature (Q.equal: the same bits, a NaN matching a NaN).  Grid points on edges and
vertices are welcome here: the highest element number wins them, in the reference and in the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import cases  # noqa: E402
import make_means_regular_golden as G  # noqa: E402
import means_regular_ref as Q  # noqa: E402
import test_gpu_means_points as TP  # noqa: E402  (the rig: one handle on a mesh with seeded accumulator rows)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "means_regular.npz")
INVALID, STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libbamg_shim.so"))
Rig, _state, _smooth_um, _lists, _free_bytes, _hip, _code, _eq = TP.Rig, TP._state, TP._smooth_um, TP._lists, TP._free_bytes, TP._hip, TP._code, TP._eq


def grid_over(x, y, ncols, nrows, reach=1.1):
    """A regular grid centred on the box of (x, y) whose extent is at least `reach` times that box in both directions."""
    spacing = 1. if ncols == nrows == 1 else max(reach * np.ptp(x) / max(ncols - 1, 1) if ncols > 1 else 0., reach * np.ptp(y) / max(nrows - 1, 1) if nrows > 1 else 0.)
    cx, cy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max())
    return dict(xmin=float(cx - 0.5 * spacing * (ncols - 1)), ymax=float(cy + 0.5 * spacing * (nrows - 1)), spacing=float(spacing), ncols=ncols, nrows=nrows)


def lon_of(g, seed=5):
    return np.random.default_rng(seed).uniform(-180., 180., g["ncols"] * g["nrows"])


def fe_set(fe, g, rotation="none", lon=None, pairs=(), miss=G.MISS):
    fe.means_regular_set(g["xmin"], g["ymax"], g["spacing"], g["ncols"], g["nrows"], miss, rotation, gridLON=lon, rotation_angle=G.ROTATION_ANGLE, pairs=pairs)


def ref_update(rig, ge, gn, g, pairs=(), cs=None, sn=None, miss=G.MISS, interp=Q.interp_mesh_to_grid):
    xd, yd = rig.x + rig.UM[:rig.nn], rig.y + rig.UM[rig.nn:]
    Q.update_grid_mean(ge, gn, xd, yd, rig.tri, rig.n_owned, rig.el, rig.nod, g, pairs, cs, sn, miss, rig.ice_col, rig.el_mask, rig.nod_mask, interp)


def chain(rig, g, rotation, pairs, UMs, lon=None, miss=G.MISS, interp=Q.interp_mesh_to_grid):
    """regular_set -> lsm -> (put_state, regular_update) per UM on the handle and in the restatement; returns (got, want) of ge, gn, lsm"""
    fe = rig.fe
    lon = lon_of(g) if lon is None else lon
    fe_set(fe, g, rotation, lon, pairs, miss)
    lsm = fe.means_regular_lsm()
    cs, sn = Q.cos_sin(rotation, G.ROTATION_ANGLE, lon)
    we, wn = rig.zeros(g["ncols"] * g["nrows"])
    for UM in UMs:
        rig.move(UM)
        fe.means_regular_update()
        ref_update(rig, we, wn, g, pairs, cs, sn, miss, interp)
    ge, gn, _, _ = fe.means_regular_get()
    return (ge, gn, lsm), (we, wn, Q.set_lsm(rig.x, rig.y, rig.tri, g, interp))


# ---- the fixture, end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    c = G.means_regular_case()
    c["z"] = dict(np.load(GOLD))
    return c


@pytest.fixture(scope="module")
def holes(case):
    c = case
    rig = Rig(c["x"], c["y"], c["tri"], c["n_owned"], c["UM1"], elemental=list(G.ELEMENTAL), nodal=list(G.NODAL), el_mask=G.EL_MASK, nod_mask=G.NOD_MASK)
    rig.el, rig.nod = c["el"], c["nod"]
    rig.inject()
    yield rig
    rig.close()


@pytest.mark.parametrize("rotation", ["none", "north_east"])
def test_fixture_end_to_end(case, holes, rotation):
    c, z, fe = case, case["z"], holes.fe
    holes.move(c["UM1"])
    fe_set(fe, G.GRID, rotation, c["lon"], G.PAIRS)
    lsm = fe.means_regular_lsm()
    assert np.array_equal(lsm, z["lsm"])
    fe.means_regular_update()
    ge, gn, _, _ = fe.means_regular_get()
    assert Q.equal(ge, z["ge1"])
    if rotation == "none":
        assert Q.equal(gn, z["gn1"])
    holes.move(c["UM2"])
    fe.means_regular_update()
    ge, gn, de, dn = fe.means_regular_get()
    assert Q.equal(ge, z["ge2"]) and Q.equal(gn, z["gn2" if rotation == "none" else "gn2_ne"])
    ge_l, gn_l, de2, dn2 = fe.means_regular_get(apply_lsm=True)
    assert Q.equal(ge_l, z["ge2_lsm"]) and (de, dn) == (de2, dn2) and de and dn
    if rotation == "north_east":
        assert Q.equal(gn_l, z["gn2_ne_lsm"])
    ge3, gn3, _, _ = fe.means_regular_get()                                      # the resident rows are unchanged by get(apply_lsm = 1) ...
    assert Q.equal(ge3, ge) and Q.equal(gn3, gn)
    raw = np.empty_like(ge)
    assert _hip().hipMemcpy(raw.ctypes.data, de, raw.nbytes, 2) == 0 and Q.equal(raw, ge)          # ... and the device pointer is theirs
    mine = (np.arange(lsm.size) % 3 != 0).astype(np.int32)                       # an uploaded mask (a partitioned run's root computed it): applied as given
    assert np.array_equal(fe.means_regular_lsm(mine), mine)
    ge_m, gn_m, _, _ = fe.means_regular_get(apply_lsm=True)
    assert Q.equal(ge_m, Q.apply_lsm(ge, mine, G.MISS)) and Q.equal(gn_m, Q.apply_lsm(gn, mine, G.MISS))


# ---- the same chain against the restatement, and against the real bamg where it was built -----------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["restatement", "real bamg"])
@pytest.mark.parametrize("kind, rotation, shape", [("tiny", "north_east", (23, 17)), ("toy", "none", (29, 37)), ("shuffled", "north_east", (37, 29))])
def test_against_the_restatement(kind, rotation, shape, interp):
    if interp == "real bamg" and not HAVE_REF:
        pytest.skip("oracle/_ref was not built: the restatement stands in for the real bamg")
    f = G.real_bamg if interp == "real bamg" else Q.interp_mesh_to_grid
    x, y, tri = TP._mesh_arrays(kind)
    um = _smooth_um(x, y, tri)
    nn = x.size
    rig = Rig(x, y, tri, tri.shape[0] - tri.shape[0] // 3, um)
    try:
        g = grid_over(x, y, *shape)
        (ge, gn, lsm), (we, wn, wl) = chain(rig, g, rotation, ((0, 1), (2, 3)), (um, np.concatenate([-3. * um[nn:], 2.5 * um[:nn]])), interp=f)
        assert Q.equal(ge, we) and Q.equal(gn, wn) and np.array_equal(lsm, wl)
        assert (lsm == 0).any() and (lsm == 1).sum() > 100 and not np.isnan(gn).any() and np.abs(gn).max() > 0
    finally:
        rig.close()


@pytest.mark.parametrize("nparts", [1, 2, 3])
def test_the_bits_of_means_to_grid_on_every_rank(nparts):
    """on zeroed accumulators with NONE, update + get is what nxs_dyn_means_to_grid, the route through the host, gives -- each rank on its own mesh"""
    gm = cases.global_mesh("small")
    um_g = _smooth_um(gm.x, gm.y, gm.tri)
    g = grid_over(gm.x, gm.y, 41, 37)
    lms = M.localize(gm, nparts, elem_part=cases.ragged_partition(gm, nparts, 7) if nparts > 1 else None)
    owned_by = np.zeros(g["ncols"] * g["nrows"], int)
    for lm in lms:
        um = np.concatenate([um_g[lm.node_gid], um_g[gm.num_nodes + lm.node_gid]])
        rig = Rig(lm.coord_x, lm.coord_y, lm.indices.reshape(-1, 3) - 1, lm.local_nelements, um, lm=lm, seed=20 + lm.rank)
        try:
            fe_set(rig.fe, g)
            rig.fe.means_regular_update()
            ge, gn, _, _ = rig.fe.means_regular_get()
            he, hn = rig.fe.means_to_grid(g["xmin"], g["ymax"], g["spacing"], g["ncols"], g["nrows"], G.MISS)
            assert Q.equal(ge, he) and Q.equal(gn, hn) and np.abs(ge).max() > 0 and np.abs(gn).max() > 0
            we, wn = rig.zeros(ge.shape[1])
            ref_update(rig, we, wn, g)
            assert Q.equal(ge, we) and Q.equal(gn, wn)
            hit = Q.find_winners(rig.x + um[:rig.nn], rig.y + um[rig.nn:], rig.tri, g)
            owned_by += (hit >= 0) & (hit < lm.local_nelements)
        finally:
            rig.close()
    assert (owned_by == 1).sum() > 500 and (nparts == 1 or owned_by.max() >= 1)


# ---- shapes where the launches can go wrong -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_xy():
    gm = cases.global_mesh("toy")
    return gm.x, gm.y, gm.tri, _smooth_um(gm.x, gm.y, gm.tri)


@pytest.fixture(scope="module")
def toy_rig(toy_xy):
    x, y, tri, um = toy_xy
    rig = Rig(x, y, tri, tri.shape[0] - 77, um)
    yield rig
    rig.close()


def _grids(x, y):
    cx, cy, wx, wy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max()), np.ptp(x), np.ptp(y)
    coarse = float(1.7 * max(wx, wy))
    return {"1x1": dict(xmin=float(cx + 0.01 * wx), ymax=float(cy - 0.02 * wy), spacing=1., ncols=1, nrows=1),
            "7x5": grid_over(x, y, 7, 5, 0.9),
            "23x17": grid_over(x, y, 23, 17, 0.95),                              # 391 points: a ragged second workgroup
            "larger on every side": grid_over(x, y, 31, 33, 1.6),
            "wholly outside": dict(xmin=float(x.max() + 0.3 * wx), ymax=float(y.min() - 0.2 * wy), spacing=float(wx / 20.), ncols=13, nrows=9),
            "much finer": dict(xmin=float(cx - 0.03 * wx), ymax=float(cy + 0.03 * wy), spacing=float(0.06 * wx / 99.), ncols=100, nrows=90),
            "much coarser": dict(xmin=float(cx + 0.05 * wx - 6 * coarse), ymax=float(cy - 0.05 * wy + 4 * coarse), spacing=coarse, ncols=13, nrows=9)}      # one point, (6, 4), near the centre


@pytest.mark.parametrize("name", ["1x1", "7x5", "23x17", "larger on every side", "wholly outside", "much finer", "much coarser"])
def test_grid_shapes(toy_xy, toy_rig, name):
    x, y, tri, um = toy_xy
    g = _grids(x, y)[name]
    (ge, gn, lsm), (we, wn, wl) = chain(toy_rig, g, "north_east", ((0, 1), (3, 2)), (um, 0.5 * um))
    assert Q.equal(ge, we) and Q.equal(gn, wn) and np.array_equal(lsm, wl), name
    hit = Q.find_winners(x + 0.5 * um[:x.size], y + 0.5 * um[x.size:], tri, g)
    if name == "wholly outside":
        assert not lsm.any() and not ge.any() and not gn.any() and (hit < 0).all()
    elif name == "much finer":
        assert lsm.all() and np.bincount(hit).max() > 300                        # a window of hundreds of points per triangle
    elif name == "much coarser":
        assert lsm.sum() == 1 and lsm.reshape(9, 13)[4, 6] == 1
    elif name == "larger on every side":
        G2 = lsm.reshape(g["nrows"], g["ncols"])
        assert not G2[0].any() and not G2[-1].any() and not G2[:, 0].any() and not G2[:, -1].any() and lsm.sum() > 200
    else:
        assert lsm.any()


@pytest.mark.parametrize("n_el, n_nod, n_pairs", [(1, 2, 1), (24, 24, 12), (5, 0, 0), (0, 6, 1), (2, 3, 0)])
def test_list_sizes(toy_xy, n_el, n_nod, n_pairs):
    """n_el = 1 and NXS_MEANS_MAX_VARS, no nodal list (no proc-mask leg), nodal only, 0 / 1 / 12 pairs"""
    x, y, tri, um = toy_xy
    rig = Rig(x, y, tri, tri.shape[0] - 77, um, n_el, n_nod)
    try:
        g = grid_over(x, y, 23, 17)
        (ge, gn, lsm), (we, wn, wl) = chain(rig, g, "north_east", tuple((2 * k, 2 * k + 1) for k in range(n_pairs)), (um,))
        assert _eq(ge, we) and _eq(gn, wn) and np.array_equal(lsm, wl)
        assert (ge is None) == (n_el == 0) and (gn is None) == (n_nod == 0)
    finally:
        rig.close()


def test_a_mesh_with_more_nodes_than_elements():
    k = 9
    x = np.concatenate([np.arange(k), np.arange(k) + 0.37]) * 1.0e4 + 3.0e5
    y = np.concatenate([np.zeros(k), np.ones(k)]) * 0.9e4 - 2.0e5 + 1.0e3 * np.sin(np.arange(2 * k))
    tri = np.array([[i, i + 1, k + i] for i in range(k - 1)] + [[i + 1, k + i + 1, k + i] for i in range(k - 1)], np.int32)
    assert x.size > tri.shape[0]
    um = _smooth_um(x, y, tri)
    rig = Rig(x, y, tri, tri.shape[0] - 5, um)
    try:
        g = grid_over(x, y, 31, 17)
        (ge, gn, lsm), (we, wn, wl) = chain(rig, g, "north_east", ((0, 1), (2, 3)), (um,))
        assert Q.equal(ge, we) and Q.equal(gn, wn) and np.array_equal(lsm, wl) and 50 < lsm.sum() < lsm.size
    finally:
        rig.close()


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_survives_set_mesh_and_regrid_reset_configure_and_removal():
    x, y, tri, ng = TP._rect()
    um = _smooth_um(x, y, tri)
    rig = Rig(x, y, tri, None, um)
    fe = rig.fe
    try:
        g = grid_over(x, y, 29, 31)
        Gn = g["ncols"] * g["nrows"]
        lon, pairs = lon_of(g), ((0, 1), (2, 3))
        cs, sn = Q.cos_sin("north_east", G.ROTATION_ANGLE, lon)
        fe_set(fe, g, "north_east", lon, pairs)
        lsm = fe.means_regular_lsm()
        fe.means_regular_update()
        we, wn = rig.zeros(Gn)
        ref_update(rig, we, wn, g, pairs, cs, sn)
        # an identity regrid (FE.cpp:8005-8010: updateGridMean just before it): the mesh accumulators start afresh, the grid ones go on
        st = _state(rig.lm, um)
        prev = np.arange(1, rig.nn + 1, dtype=np.float64)
        fe.regrid(rig.lm, prev, ng, {k: st[k] for k in dynamics.REGRID_INPUTS}, (), moved=(rig.lm.coord_x, rig.lm.coord_y))
        el0, nod0, _, _ = fe.means_get()
        assert not el0.any() and not nod0.any()
        rig.move(0.5 * um)
        rig.seed_rows(12)
        fe.means_regular_update()
        ref_update(rig, we, wn, g, pairs, cs, sn)
        ge, gn, _, _ = fe.means_regular_get()
        assert Q.equal(ge, we) and Q.equal(gn, wn)
        # ... and another mesh altogether: the grid, the mask and the accumulators are still there
        gm2 = cases.global_mesh("tiny")
        rig2 = Rig.__new__(Rig)
        rig2.__dict__.update(rig.__dict__)
        rig2.x, rig2.y, rig2.tri = gm2.x, gm2.y, gm2.tri
        rig2.nn, rig2.ne, rig2.n_owned = gm2.num_nodes, gm2.num_elements, gm2.num_elements
        rig2.lm = M.localize(gm2, 1)[0]
        fe.set_mesh(rig2.lm)
        rig2.move(np.zeros(2 * rig2.nn))
        fe.means_update(1.0)
        rig2.seed_rows(13)
        assert np.array_equal(fe.means_regular_get(apply_lsm=True)[0][0] == G.MISS, lsm == 0)
        fe.means_regular_update()
        ge2, gn2, _, _ = fe.means_regular_get()
        ref_update(rig2, we, wn, g, pairs, cs, sn)
        assert Q.equal(ge2, we) and Q.equal(gn2, wn)
        # reset
        fe.means_regular_reset()
        ge, gn, _, _ = fe.means_regular_get()
        assert not ge.view(np.uint64).any() and not gn.view(np.uint64).any()
        # configure with other list sizes: the accumulators are made again at the new sizes, zeroed; the grid and the mask stay
        fe.means_regular_update()
        fe.means_configure(("conc", "ice_mask"), ("VT_x", "VT_y"))
        ge, gn, _, _ = fe.means_regular_get()
        assert ge.shape == (2, Gn) and gn.shape == (2, Gn) and not ge.any() and not gn.any()
        assert np.array_equal(fe.means_regular_get(apply_lsm=True)[1][1] == G.MISS, lsm == 0)
        code, text = _code(fe.means_regular_update)                               # the pair (2, 3) is outside the new nodal list
        assert code == STATE and "pair 1" in text
        # removal
        free0 = _free_bytes()
        fe.means_regular_set()
        assert _free_bytes() >= free0
        assert _code(fe.means_regular_update)[0] == STATE and _code(fe.means_regular_get)[0] == STATE and _code(fe.means_regular_reset)[0] == STATE
        assert _code(fe.means_regular_lsm)[0] == STATE
    finally:
        rig.close()


def test_handles_give_their_memory_back(toy_xy):
    """four cycles of create / set / lsm / update / get / destroy leave the free device memory where it settled; a removed grid gives back what it took"""
    x, y, tri, um = toy_xy
    g = grid_over(x, y, 400, 400)                                                # 160 000 points: 9 MB of accumulators, 3 MB of angles and winners
    lon = lon_of(g)
    free = []
    for cycle in range(4):
        rig = Rig(x, y, tri, None, um)
        rig.fe.synchronize()
        before = _free_bytes()
        fe_set(rig.fe, g, "north_east", lon, ((0, 1),))
        rig.fe.means_regular_lsm()
        rig.fe.means_regular_update()
        rig.fe.means_regular_get()
        rig.fe.synchronize()
        if cycle == 3:
            rig.fe.means_regular_set()
            assert _free_bytes() >= before, (before, _free_bytes())
        rig.close()
        free.append(_free_bytes())
    assert free[1] == free[2] == free[3], free


def test_a_handle_that_never_calls_them_allocates_nothing(toy_xy):
    x, y, tri, um = toy_xy
    rig = Rig(x, y, tri, None, um)
    try:
        rig.fe.synchronize()
        free0 = _free_bytes()
        rig.fe.means_update(1.0); rig.fe.means_get(); rig.fe.means_reset(); rig.fe.means_update(1.0)
        rig.fe.synchronize()
        assert _free_bytes() == free0
        rig.fe.means_configure(*_lists(2, 2)[:2])                                # (other list sizes: there are no grid accumulators to drop)
        rig.fe.means_update(1.0)
        assert _code(rig.fe.means_regular_get)[0] == STATE
    finally:
        rig.close()


# ---- neighbours untouched -------------------------------------------------------------------------------------------------------------------------------------
def test_after_a_step_and_beside_the_drifters_and_the_loaded_grid():
    gm, p, g_, lms, fields = cases.make_case("toy")
    lm, f = lms[0], fields[0]
    tri = lm.indices.reshape(-1, 3) - 1
    nn = lm.num_nodes
    elemental, nodal = ("conc", ("thick", True), "ice_mask"), ("VT_x", ("VT_y", True), "tau_ax", "tau_ay")
    import make_means_points_golden as GP
    gx, gy, plon, theta = GP.curvilinear_grid(lm.coord_x, lm.coord_y, 31, 27, seed=2)
    g = grid_over(lm.coord_x, lm.coord_y, 41, 37)
    lon, pairs = lon_of(g), ((0, 1), (2, 3))
    rng = np.random.default_rng(1)
    dx, dy = lm.coord_x.min() + np.ptp(lm.coord_x) * rng.random(500), lm.coord_y.min() + np.ptp(lm.coord_y) * rng.random(500)
    ids = np.arange(500, dtype=np.int32)

    def run(with_regular):
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
        fe.means_configure(elemental, nodal)
        fe.means_points_set(gx, gy, G.MISS, "north_east", gridLON=plon, rotation_angle=G.ROTATION_ANGLE, pairs=pairs)
        out = {}
        if with_regular:
            fe_set(fe, g, "north_east", lon, pairs)
            fe.means_regular_lsm()
        fe.means_update(1.0)
        if with_regular:
            fe.means_regular_update()
        fe.step()
        fe.means_update(1.0)
        fe.drifters_set(0, dx, dy, ids)
        out["conc_before"] = fe.drifters_conc(0)
        if with_regular:
            um1 = fe.get_state()["UM"]
            assert not np.array_equal(f["UM"], um1)
            el, nod, _, _ = fe.means_get()
            before_e, before_n, _, _ = fe.means_regular_get()
            fe.means_regular_update()                                            # sees the new M_UM
            ge, gn, _, _ = fe.means_regular_get()
            cs, sn = Q.cos_sin("north_east", G.ROTATION_ANGLE, lon)
            Q.update_grid_mean(before_e, before_n, lm.coord_x + um1[:nn], lm.coord_y + um1[nn:], tri, lm.local_nelements, el, nod, g, pairs, cs, sn, G.MISS, 2, (0, 1, 0), (0, 1, 0, 0))
            assert Q.equal(ge, before_e) and Q.equal(gn, before_n) and np.abs(gn).max() > 0
            el2, nod2, _, _ = fe.means_get()
            assert Q.equal(el2, el) and Q.equal(nod2, nod)                       # the mesh accumulators are only read
        out["conc_after"] = fe.drifters_conc(0)
        fe.means_points_update()
        out["points"] = fe.means_points_get()[:2]
        out["state"] = fe.get_state()
        fe.close()
        return out
    a, b = run(True), run(False)
    assert np.array_equal(a["conc_before"], a["conc_after"]) and np.array_equal(a["conc_before"], b["conc_before"]) and np.array_equal(b["conc_after"], b["conc_before"])
    assert Q.equal(a["points"][0], b["points"][0]) and Q.equal(a["points"][1], b["points"][1]) and np.abs(a["points"][1]).max() > 0
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k]), k


# ---- error paths ----------------------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_texts(toy_xy):
    x, y, tri, um = toy_xy
    g = grid_over(x, y, 11, 13)
    Gn = 11 * 13
    lon = lon_of(g)
    fe = dynamics.FiniteElementDynamics(F.default_params(), device=0)
    try:
        code, text = _code(fe.means_regular_update)
        assert code == STATE and "set_mesh" in text
        assert _code(fe.means_regular_lsm)[0] == STATE and "no grid" in _code(fe.means_regular_get)[1] and _code(fe.means_regular_reset)[0] == STATE
        code, text = _code(fe_set, fe, g, pairs=((0, 1),))                        # nothing configured: no nodal list to name a column of
        assert code == INVALID and "pair 0" in text
        fe_set(fe, g)                                                             # (legal before set_mesh: the grid does not depend on the mesh)
        assert _code(fe.means_regular_lsm)[0] == STATE and "set_mesh" in _code(fe.means_regular_lsm)[1]
        assert np.array_equal(fe.means_regular_lsm(np.ones(Gn, np.int32)), np.ones(Gn, np.int32))
        lm = M.localize(TP._global_mesh(x, y, tri), 1)[0]
        fe.set_mesh(lm)
        assert _code(fe.means_regular_update)[0] == STATE                         # no state
        fe.put_state(_state(lm, um))
        code, text = _code(fe.means_regular_update)
        assert code == STATE and "no variable is configured" in text
        assert _code(fe.means_regular_get)[0] == STATE and "no variable is configured" in _code(fe.means_regular_get)[1]
        fe.means_configure(*_lists(3, 4)[:2])
        for kw, word in ((dict(pairs=((0, 4),)), "pair 0"), (dict(pairs=((-1, 0),)), "pair 0"), (dict(pairs=tuple((0, 1) for _ in range(13))), "n_pairs"),
                         (dict(rotation="north_east"), "gridLON"), (dict(rotation="grid_theta", lon=lon), "GRID_THETA"), (dict(rotation=7), "rotation")):
            code, text = _code(fe_set, fe, g, **kw)
            assert code == INVALID and word in text, (kw, text)
        for over, word in ((dict(spacing=0.), "mooring_spacing"), (dict(spacing=-2.), "mooring_spacing"), (dict(spacing=np.nan), "mooring_spacing"), (dict(xmin=np.inf), "not finite"),
                           (dict(ymax=np.nan), "not finite"), (dict(ncols=-3), "ncols = -3"), (dict(nrows=-1), "nrows = -1"), (dict(ncols=70000, nrows=70000), "do not fit")):
            code, text = _code(fe_set, fe, dict(g, **over))
            assert code == INVALID and word in text, (over, text)
        bad = lon.copy(); bad[3] = np.nan
        code, text = _code(fe_set, fe, g, "north_east", bad)
        assert code == INVALID and "grid point 3" in text
        # a refused set leaves the previous grid, and the handle works
        fe.means_regular_update()
        ge, gn, _, _ = fe.means_regular_get(apply_lsm=True)
        assert ge.shape == (3, Gn) and gn.shape == (4, Gn)
    finally:
        fe.close()
