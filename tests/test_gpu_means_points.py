"""The Moorings means on a LOADED grid on the device (nxs_dyn_means_points_*): GridOutput::updateGridMean through the M_grid.loaded, non-conservative branch, rotateVectors,
setLSM / applyLSM, resetGridMean (model/gridoutput.cpp:387-415, 470-485, 558-651) on the handle's own accumulators, against the fixture the real contrib/bamg wrote
(tests/golden/means_points.npz) and the restatement tests/means_points_ref.py.  Bit for bit: there is no tolerance anywhere in this feature (P.equal: the same bits,
a NaN matching a NaN).  Every comparison first asserts that its own inputs have no grid point on an edge or a vertex (the one case where the reference's own
answer depends on its triangle walk)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import cases  # noqa: E402
import make_means_points_golden as G  # noqa: E402
import means_points_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "means_points.npz")
INVALID, STATE = -1, -4
EL_CYCLE = ("conc", "thick", "snow", "damage", "ridge_ratio", "conc_cons")
NOD_CYCLE = ("VT_x", "VT_y", "tau_ax", "tau_ay")


def _hip():
    L = dynamics.load_library()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemcpy.restype = C.c_int
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    return L


def _free_bytes():
    a, b = C.c_size_t(), C.c_size_t()
    assert _hip().hipMemGetInfo(C.byref(a), C.byref(b)) == 0
    return a.value


def _global_mesh(x, y, tri, name="holes"):
    e = np.concatenate([tri[:, [1, 2]], tri[:, [2, 0]], tri[:, [0, 1]]], 0).astype(np.int64)
    key = np.sort(e, 1)[:, 0] * x.size + np.sort(e, 1)[:, 1]
    uk, first, cnt = np.unique(key, return_index=True, return_counts=True)
    coast = np.zeros(x.size, bool); coast[e[first[cnt == 1]].ravel()] = True
    return M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=coast,
                        neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name=name)


def _state(lm, UM, seed=3):
    """A full prognostic state on one rank: UM as given (local numbering), everything else seeded noise."""
    rng = np.random.default_rng(seed)
    s = {k: rng.standard_normal(2 * lm.num_nodes) for k in _abi.STATE_NODAL}
    s.update({k: rng.random(lm.num_elements) for k in _abi.STATE_ELEMENT + _abi.STATE_INPUT})
    s["UM"] = np.ascontiguousarray(UM, np.float64)
    return s


def _smooth_um(x, y, tri, scale=0.04):
    xs, ys = x[tri], y[tri]
    area = 0.5 * np.abs((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0]))
    h, L = float(np.sqrt(2. * area.min())), max(np.ptp(x), np.ptp(y))
    return np.concatenate([scale * h * np.sin(3. * x / L) * np.cos(2. * y / L + 0.1), scale * h * np.cos(2. * x / L + 0.7) * np.sin(3. * y / L)])


def _lists(n_el, n_nod, masks=True):
    """configure() lists of the sizes asked for out of variables that need neither a step nor a forcing; ice_mask last among the elemental ones"""
    el = [EL_CYCLE[k % len(EL_CYCLE)] for k in range(max(n_el - 1, 0))] + (["ice_mask"] if n_el else [])
    el_mask = [int(masks and k % 2 == 1 and n_el > 1) for k in range(n_el)]
    if n_el:
        el_mask[-1] = 0
    nod = [NOD_CYCLE[k % 4] for k in range(n_nod)]
    nod_mask = [int(masks and k % 3 == 1 and n_el > 0) for k in range(n_nod)]
    return [(n, bool(m)) for n, m in zip(el, el_mask)], [(n, bool(m)) for n, m in zip(nod, nod_mask)], el_mask, nod_mask


class Rig:
    """One handle on a mesh (x, y, tri 0-based, the first n_owned elements owned) with seeded accumulator rows written over what means_update made."""

    def __init__(self, x, y, tri, n_owned=None, UM=None, n_el=3, n_nod=4, seed=11, lm=None, elemental=None, nodal=None, el_mask=None, nod_mask=None):
        self.x, self.y, self.tri = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(tri)
        self.ne, self.nn = self.tri.shape[0], self.x.size
        self.n_owned = self.ne if n_owned is None else n_owned
        if lm is None:
            lm = M.localize(_global_mesh(self.x, self.y, self.tri), 1)[0]
            assert np.array_equal(lm.indices.reshape(-1, 3) - 1, self.tri) and np.array_equal(lm.coord_x, self.x)
            lm = dataclasses.replace(lm, local_nelements=self.n_owned)
        self.lm = lm
        self.UM = np.zeros(2 * self.nn) if UM is None else UM
        if elemental is None:
            elemental, nodal, el_mask, nod_mask = _lists(n_el, n_nod)
        self.el_mask, self.nod_mask = list(el_mask), list(nod_mask)
        self.n_el, self.n_nod = len(elemental), len(nodal)
        names = [v if isinstance(v, str) else v[0] for v in elemental]
        self.ice_col = names.index("ice_mask") if "ice_mask" in names else -1
        self.fe = dynamics.FiniteElementDynamics(F.default_params(), device=0)
        self.fe.set_mesh(lm)
        self.fe.means_configure(elemental, nodal)
        self.fe.put_state(_state(lm, self.UM))
        self.fe.means_update(1.0)
        self.seed_rows(seed)

    def seed_rows(self, seed):
        rng = np.random.default_rng(seed)
        self.el = rng.normal(0., 1., (self.ne, self.n_el))
        if self.n_el:
            self.el[:, -1] = rng.integers(-1, 3, self.ne)
            self.el[self.n_owned:] = 0.
            self.el[rng.integers(0, self.ne)] = 0.
        self.nod = rng.normal(0., 5., (self.nn, self.n_nod))
        if self.n_nod:
            self.nod[rng.integers(0, self.nn)] = np.nan
        self.inject()

    def inject(self):
        _, _, de, dn = self.fe.means_get(want_host=False)
        for a, p in ((self.el, de), (self.nod, dn)):
            if a.size:
                assert p and _hip().hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0

    def move(self, UM):
        self.UM = UM
        st = _state(self.lm, UM)
        self.fe.put_state(st)

    def ref_update(self, ge, gn, gx, gy, pairs=(), cs=None, sn=None, miss=G.MISS):
        xd, yd = self.x + self.UM[:self.nn], self.y + self.UM[self.nn:]
        assert P.ties(xd, yd, self.tri, gx, gy) == 0
        P.update_grid_mean(ge, gn, xd, yd, self.tri, self.n_owned, self.el, self.nod, gx, gy, pairs, cs, sn, miss, self.ice_col, self.el_mask, self.nod_mask)

    def zeros(self, Gn):
        return (np.zeros((self.n_el, Gn)) if self.n_el else None), (np.zeros((self.n_nod, Gn)) if self.n_nod else None)

    def close(self):
        self.fe.close()


def _eq(a, b):
    return (a is None and b is None) or P.equal(a, b)


def _code(fn, *a, **k):
    with pytest.raises(dynamics.NxsError) as e:
        fn(*a, **k)
    return e.value.code, str(e.value)


# ---- the fixture, end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    c = G.means_points_case()
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


@pytest.mark.parametrize("rotation", ["north_east", "grid_theta"])
def test_fixture_end_to_end(case, holes, rotation):
    c, z, fe = case, case["z"], holes.fe
    assert G.ties(c) == (0, 0, 0)
    holes.move(c["UM1"])
    fe.means_points_set(c["gx"], c["gy"], G.MISS, rotation, gridLON=c["lon"], gridTheta=c["theta"], rotation_angle=G.ROTATION_ANGLE, pairs=G.PAIRS)
    lsm = fe.means_points_lsm()
    assert np.array_equal(lsm, z["lsm"])
    fe.means_points_update()
    ge, gn, _, _ = fe.means_points_get()
    if rotation == "north_east":
        assert P.equal(ge, z["ge1"]) and P.equal(gn, z["gn1"])
    holes.move(c["UM2"])
    fe.means_points_update()
    ge, gn, de, dn = fe.means_points_get()
    assert P.equal(ge, z["ge2"]) and P.equal(gn, z["gn2" if rotation == "north_east" else "gn2_theta"])
    if rotation == "north_east":
        ge_l, gn_l, de2, dn2 = fe.means_points_get(apply_lsm=True)
        assert P.equal(ge_l, z["ge2_lsm"]) and P.equal(gn_l, z["gn2_lsm"]) and (de, dn) == (de2, dn2) and de and dn
        ge3, gn3, _, _ = fe.means_points_get()                                  # the resident rows are unchanged by get(apply_lsm = 1) ...
        assert P.equal(ge3, ge) and P.equal(gn3, gn)
        raw = np.empty_like(ge)
        assert _hip().hipMemcpy(raw.ctypes.data, de, raw.nbytes, 2) == 0 and P.equal(raw, ge)      # ... and the device pointer is theirs
        # an uploaded mask (a partitioned run's root computed it): applied as given
        mine = (np.arange(lsm.size) % 3 != 0).astype(np.int32)
        assert np.array_equal(fe.means_points_lsm(mine), mine)
        ge_m, gn_m, _, _ = fe.means_points_get(apply_lsm=True)
        assert P.equal(ge_m, P.apply_lsm(ge, mine, G.MISS)) and P.equal(gn_m, P.apply_lsm(gn, mine, G.MISS))


# ---- the same chain against the restatement: other meshes, a shuffled numbering, real partitions --------------------------------------------------------------
def _mesh_arrays(kind):
    if kind == "shuffled":
        g0 = cases.global_mesh("small")
        rng = np.random.default_rng(7)
        pn, pe = rng.permutation(g0.num_nodes), rng.permutation(g0.num_elements)
        inv = np.empty_like(pn); inv[pn] = np.arange(pn.size)
        return g0.x[pn].copy(), g0.y[pn].copy(), np.ascontiguousarray(inv[g0.tri][pe].astype(np.int32))
    gm = cases.global_mesh(kind)
    return gm.x, gm.y, gm.tri


def _chain(rig, gx, gy, lon, theta, rotation, pairs, UMs, miss=G.MISS):
    """points_set -> lsm -> (put_state, points_update) per UM on the handle and in the restatement; returns (got, want) of ge, gn, lsm"""
    fe = rig.fe
    fe.means_points_set(gx, gy, miss, rotation, gridLON=lon, gridTheta=theta, rotation_angle=G.ROTATION_ANGLE, pairs=pairs)
    assert P.ties(rig.x, rig.y, rig.tri, gx, gy) == 0
    lsm = fe.means_points_lsm()
    cs, sn = P.cos_sin(rotation, G.ROTATION_ANGLE, lon, theta)
    we, wn = rig.zeros(gx.size)
    for UM in UMs:
        rig.move(UM)
        fe.means_points_update()
        rig.ref_update(we, wn, gx, gy, pairs, cs, sn, miss)
    ge, gn, _, _ = fe.means_points_get()
    return (ge, gn, lsm), (we, wn, P.set_lsm(rig.x, rig.y, rig.tri, gx, gy))


@pytest.mark.parametrize("kind, rotation", [("tiny", "north_east"), ("toy", "grid_theta"), ("shuffled", "north_east"), ("toy", "none")])
def test_against_the_restatement(kind, rotation):
    x, y, tri = _mesh_arrays(kind)
    um = _smooth_um(x, y, tri)
    nn = x.size
    rig = Rig(x, y, tri, tri.shape[0] - tri.shape[0] // 3, um)
    try:
        gx, gy, lon, theta = G.curvilinear_grid(x, y, 37, 29, seed=3)
        (ge, gn, lsm), (we, wn, wl) = _chain(rig, gx, gy, lon, theta, rotation, ((0, 1), (2, 3)), (um, np.concatenate([-3. * um[nn:], 2.5 * um[:nn]])))
        assert P.equal(ge, we) and P.equal(gn, wn) and np.array_equal(lsm, wl)
        assert (lsm == 0).any() and (lsm == 1).sum() > 100 and np.isnan(gn).any() == np.isnan(wn).any()
    finally:
        rig.close()


@pytest.mark.parametrize("nparts", [2, 3])
def test_partitioned_handles_each_against_their_own_mesh(nparts):
    """what the reference's per-rank call does: the rank's own box, its own integer plane, its ghosts at the end"""
    gm = cases.global_mesh("small")
    um_g = _smooth_um(gm.x, gm.y, gm.tri)
    gx, gy, lon, theta = G.curvilinear_grid(gm.x, gm.y, 37, 29, seed=4)
    found_by, in_a_ghost = np.zeros(gx.size, int), 0
    lms = M.localize(gm, nparts, elem_part=cases.ragged_partition(gm, nparts, 7))
    assert any(0 < lm.local_nelements < lm.num_elements for lm in lms)
    for lm in lms:
        um = np.concatenate([um_g[lm.node_gid], um_g[gm.num_nodes + lm.node_gid]])
        rig = Rig(lm.coord_x, lm.coord_y, lm.indices.reshape(-1, 3) - 1, lm.local_nelements, um, lm=lm, seed=20 + lm.rank)
        try:
            (ge, gn, lsm), (we, wn, wl) = _chain(rig, gx, gy, lon, theta, "north_east", ((0, 1), (2, 3)), (um,))
            assert P.equal(ge, we) and P.equal(gn, wn) and np.array_equal(lsm, wl)
            it, _ = P.R.locate(rig.x + um[:rig.nn], rig.y + um[rig.nn:], rig.tri, gx, gy)
            found_by += (it >= 0) & (it < lm.local_nelements)
            in_a_ghost += int((it >= lm.local_nelements).sum())
        finally:
            rig.close()
    assert found_by.max() == 1 and (found_by == 1).sum() > 500 and in_a_ghost > 0      # every point of the sea belongs to exactly one rank's proc mask


# ---- shapes where the launch can go wrong ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_xy():
    gm = cases.global_mesh("toy")
    return gm.x, gm.y, gm.tri, _smooth_um(gm.x, gm.y, gm.tri)


@pytest.mark.parametrize("n_el, n_nod, n_pairs", [(3, 4, 2), (1, 2, 1), (24, 24, 12), (5, 0, 0), (0, 6, 1), (2, 3, 0)])
def test_list_sizes_and_grid_sizes(toy_xy, n_el, n_nod, n_pairs):
    """n_el = 1 and NXS_MEANS_MAX_VARS, no nodal list (no proc-mask leg), nodal only, 0 / 1 / 12 pairs; G = 1, 255, 256, 257"""
    x, y, tri, um = toy_xy
    rig = Rig(x, y, tri, tri.shape[0] - 77, um, n_el, n_nod)
    try:
        gx, gy, lon, theta = G.curvilinear_grid(x, y, 23, 19, seed=5)
        pairs = tuple((2 * k, 2 * k + 1) for k in range(n_pairs))
        for Gn in (1, 255, 256, 257):
            sel = slice(60, 60 + Gn)
            (ge, gn, lsm), (we, wn, wl) = _chain(rig, gx[sel], gy[sel], lon[sel], theta[sel], "grid_theta", pairs, (um,))
            assert _eq(ge, we) and _eq(gn, wn) and np.array_equal(lsm, wl), Gn
            assert (ge is None) == (n_el == 0) and (gn is None) == (n_nod == 0)
    finally:
        rig.close()


def test_every_point_outside_the_box_and_every_point_in_one_element(toy_xy):
    x, y, tri, um = toy_xy
    rig = Rig(x, y, tri, tri.shape[0] - 77, um)
    try:
        rng = np.random.default_rng(9)
        n = 300
        far = (x.max() + np.ptp(x) * (0.01 + rng.random(n)), y.min() + np.ptp(y) * rng.random(n))
        e = 5
        w = rng.dirichlet((1., 1., 1.), n) * 0.94 + 0.02
        xd, yd = x + um[:x.size], y + um[x.size:]
        one = ((w * xd[tri[e]]).sum(1), (w * yd[tri[e]]).sum(1))
        for name, (gx, gy) in (("outside", far), ("one element", one)):
            gx, gy = np.ascontiguousarray(gx), np.ascontiguousarray(gy)
            z = np.zeros(n)
            (ge, gn, lsm), (we, wn, wl) = _chain(rig, gx, gy, z + 10., z + 0.3, "north_east", ((0, 1), (3, 2)), (um, um))
            assert P.equal(ge, we) and P.equal(gn, wn) and np.array_equal(lsm, wl), name
            if name == "outside":
                assert not ge.any() and not gn.any() and not lsm.any()           # 0. + 0. twice; the masked ones 0. by the rule as well
            else:
                assert np.array_equal(ge[0], np.full(n, rig.el[e, 0] + rig.el[e, 0])) and lsm.sum() > n // 2
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
        gx, gy, lon, theta = G.curvilinear_grid(x, y, 31, 17, seed=6)
        (ge, gn, lsm), (we, wn, wl) = _chain(rig, gx, gy, lon, theta, "north_east", ((0, 1), (2, 3)), (um,))
        assert P.equal(ge, we) and P.equal(gn, wn) and np.array_equal(lsm, wl) and 50 < lsm.sum() < lsm.size
    finally:
        rig.close()


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------------------------------
def _rect():
    x, y, tri, ng = cases.rect_mesh(25, 1)
    return np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64), np.ascontiguousarray(tri, np.int32), ng


def test_the_grid_survives_set_mesh_and_regrid_reset_configure_and_removal():
    x, y, tri, ng = _rect()
    um = _smooth_um(x, y, tri)
    rig = Rig(x, y, tri, None, um)
    fe = rig.fe
    try:
        gx, gy, lon, theta = G.curvilinear_grid(x, y, 29, 31, seed=8)
        pairs = ((0, 1), (2, 3))
        cs, sn = P.cos_sin("north_east", G.ROTATION_ANGLE, lon, theta)
        fe.means_points_set(gx, gy, G.MISS, "north_east", gridLON=lon, rotation_angle=G.ROTATION_ANGLE, pairs=pairs)
        lsm = fe.means_points_lsm()
        fe.means_points_update()
        we, wn = rig.zeros(gx.size)
        rig.ref_update(we, wn, gx, gy, pairs, cs, sn)
        # an identity regrid (FE.cpp:9471: updateGridMean just before it): the mesh accumulators start afresh, the grid ones go on
        st = _state(rig.lm, um)
        prev = np.arange(1, rig.nn + 1, dtype=np.float64)
        inputs = {k: st[k] for k in dynamics.REGRID_INPUTS}
        fe.regrid(rig.lm, prev, ng, inputs, (), moved=(rig.lm.coord_x, rig.lm.coord_y))
        el0, nod0, _, _ = fe.means_get()
        assert not el0.any() and not nod0.any()
        um2 = 0.5 * um
        rig.move(um2)
        rig.seed_rows(12)
        fe.means_points_update()
        rig.ref_update(we, wn, gx, gy, pairs, cs, sn)
        ge, gn, _, _ = fe.means_points_get()
        assert P.equal(ge, we) and P.equal(gn, wn)
        # ... and another mesh altogether: the points, the mask and the accumulators are still there
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
        assert np.array_equal(fe.means_points_get(apply_lsm=True)[0][0] == G.MISS, lsm == 0)
        fe.means_points_update()
        ge2, gn2, _, _ = fe.means_points_get()
        rig2.ref_update(we, wn, gx, gy, pairs, cs, sn)
        assert P.equal(ge2, we) and P.equal(gn2, wn)
        # reset
        fe.means_points_reset()
        ge, gn, _, _ = fe.means_points_get()
        assert not ge.view(np.uint64).any() and not gn.view(np.uint64).any()
        # configure with other list sizes: the accumulators are made again at the new sizes, zeroed; the points and the mask stay
        fe.means_points_update()
        fe.means_configure(("conc", "ice_mask"), ("VT_x", "VT_y"))
        ge, gn, _, _ = fe.means_points_get()
        assert ge.shape == (2, gx.size) and gn.shape == (2, gx.size) and not ge.any() and not gn.any()
        assert np.array_equal(fe.means_points_get(apply_lsm=True)[1][1] == G.MISS, lsm == 0)
        code, text = _code(fe.means_points_update)                               # the pair (2, 3) is outside the new nodal list
        assert code == STATE and "pair 1" in text
        # removal
        free0 = _free_bytes()
        fe.means_points_set()
        assert _free_bytes() >= free0
        assert _code(fe.means_points_update)[0] == STATE and _code(fe.means_points_get)[0] == STATE and _code(fe.means_points_reset)[0] == STATE
        assert _code(fe.means_points_lsm)[0] == STATE
    finally:
        rig.close()


def test_handles_give_their_memory_back(toy_xy):
    """four cycles of create / set / lsm / update / get / destroy leave the free device memory where it settled; a removed grid gives back what it took"""
    x, y, tri, um = toy_xy
    gx, gy, lon, theta = G.curvilinear_grid(x, y, 400, 400, seed=5)      # 160 000 points: 9 MB of accumulators, 5 MB of coordinates and angles
    free = []
    for cycle in range(4):
        rig = Rig(x, y, tri, None, um)
        before = _free_bytes()
        rig.fe.means_points_set(gx, gy, G.MISS, "grid_theta", gridTheta=theta, pairs=((0, 1),))
        rig.fe.means_points_lsm()
        rig.fe.means_points_update()
        rig.fe.means_points_get()
        rig.fe.synchronize()
        if cycle == 3:
            rig.fe.drifters_clear(0)
            rig.fe.means_points_set()
            after = _free_bytes()
            assert after >= before - (4 << 20), (before, after)                  # (what stays is the drifters' locator, made by the first call that needs one)
        rig.close()
        free.append(_free_bytes())
    assert free[1] == free[2] == free[3], free


# ---- neighbours untouched -------------------------------------------------------------------------------------------------------------------------------------
def test_after_a_step_and_beside_the_drifters_and_the_regular_grid():
    gm, p, g, lms, fields = cases.make_case("toy")
    lm, f = lms[0], fields[0]
    tri = lm.indices.reshape(-1, 3) - 1
    nn = lm.num_nodes
    elemental, nodal = ("conc", ("thick", True), "ice_mask"), ("VT_x", ("VT_y", True), "tau_ax", "tau_ay")
    gx, gy, lon, theta = G.curvilinear_grid(lm.coord_x, lm.coord_y, 31, 27, seed=2)
    rng = np.random.default_rng(1)
    dx, dy = lm.coord_x.min() + np.ptp(lm.coord_x) * rng.random(500), lm.coord_y.min() + np.ptp(lm.coord_y) * rng.random(500)
    ids = np.arange(500, dtype=np.int32)
    grid_args = (float(lm.coord_x.min()), float(lm.coord_y.max()), float(np.ptp(lm.coord_x) / 40.), 41, 37)

    def run(with_points):
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
        fe.means_configure(elemental, nodal)
        out = {}
        if with_points:
            fe.means_points_set(gx, gy, G.MISS, "north_east", gridLON=lon, rotation_angle=G.ROTATION_ANGLE, pairs=((0, 1), (2, 3)))
            fe.means_points_lsm()
        fe.means_update(1.0)
        if with_points:
            fe.means_points_update()                                             # (builds the displaced locator before the step)
        fe.step()
        fe.means_update(1.0)
        fe.drifters_set(0, dx, dy, ids)
        out["conc_before"] = fe.drifters_conc(0)
        if with_points:
            um0 = f["UM"]
            um1 = fe.get_state()["UM"]
            assert not np.array_equal(um0, um1)
            el, nod, _, _ = fe.means_get()
            before_e, before_n, _, _ = fe.means_points_get()
            fe.means_points_update()                                             # sees the new M_UM: the locator is rebuilt
            ge, gn, _, _ = fe.means_points_get()
            xd, yd = lm.coord_x + um1[:nn], lm.coord_y + um1[nn:]
            assert P.ties(xd, yd, tri, gx, gy) == 0
            cs, sn = P.cos_sin("north_east", G.ROTATION_ANGLE, lon, theta)
            P.update_grid_mean(before_e, before_n, xd, yd, tri, lm.local_nelements, el, nod, gx, gy, ((0, 1), (2, 3)), cs, sn, G.MISS, 2, (0, 1, 0), (0, 1, 0, 0))
            assert P.equal(ge, before_e) and P.equal(gn, before_n) and np.abs(gn).max() > 0
            el2, nod2, _, _ = fe.means_get()
            assert P.equal(el2, el) and P.equal(nod2, nod)                       # the mesh accumulators are only read
        out["conc_after"] = fe.drifters_conc(0)
        out["grid"] = fe.means_to_grid(*grid_args)
        out["state"] = fe.get_state()
        fe.close()
        return out
    a, b = run(True), run(False)
    assert np.array_equal(a["conc_before"], a["conc_after"]) and np.array_equal(a["conc_before"], b["conc_before"]) and np.array_equal(b["conc_after"], b["conc_before"])
    assert P.equal(a["grid"][0], b["grid"][0]) and P.equal(a["grid"][1], b["grid"][1]) and np.abs(a["grid"][1]).max() > 0
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k]), k


def test_a_handle_that_never_calls_them_allocates_nothing(toy_xy):
    x, y, tri, um = toy_xy
    rig = Rig(x, y, tri, None, um)
    try:
        rig.fe.synchronize()
        free0 = _free_bytes()
        rig.fe.means_update(1.0); rig.fe.means_get(); rig.fe.means_reset(); rig.fe.means_update(1.0)
        rig.fe.synchronize()
        assert _free_bytes() == free0
    finally:
        rig.close()


# ---- error paths ----------------------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_texts(toy_xy):
    x, y, tri, um = toy_xy
    gx, gy, lon, theta = G.curvilinear_grid(x, y, 11, 13, seed=5)
    fe = dynamics.FiniteElementDynamics(F.default_params(), device=0)
    try:
        code, text = _code(fe.means_points_update)
        assert code == STATE and "set_mesh" in text
        assert _code(fe.means_points_lsm)[0] == STATE and "no grid points" in _code(fe.means_points_get)[1] and _code(fe.means_points_reset)[0] == STATE
        code, text = _code(fe.means_points_set, gx, gy, pairs=((0, 1),))          # nothing configured: no nodal list to name a column of
        assert code == INVALID and "pair 0" in text
        fe.means_points_set(gx, gy)                                               # (legal before set_mesh: the grid does not depend on the mesh)
        assert _code(fe.means_points_lsm)[0] == STATE and "set_mesh" in _code(fe.means_points_lsm)[1]
        assert np.array_equal(fe.means_points_lsm(np.ones(gx.size, np.int32)), np.ones(gx.size, np.int32))
        lm = M.localize(_global_mesh(x, y, tri), 1)[0]
        fe.set_mesh(lm)
        assert _code(fe.means_points_update)[0] == STATE                          # no state
        fe.put_state(_state(lm, um))
        code, text = _code(fe.means_points_update)
        assert code == STATE and "no variable is configured" in text
        assert _code(fe.means_points_get)[0] == STATE
        fe.means_configure(*_lists(3, 4)[:2])
        for kw, word in ((dict(pairs=((0, 4),)), "pair 0"), (dict(pairs=((-1, 0),)), "pair 0"), (dict(pairs=tuple((0, 1) for _ in range(13))), "n_pairs"),
                         (dict(rotation="north_east"), "gridLON"), (dict(rotation="grid_theta", gridLON=lon), "gridTheta"), (dict(rotation=7), "rotation")):
            code, text = _code(fe.means_points_set, gx, gy, **kw)
            assert code == INVALID and word in text, (kw, text)
        bad = gx.copy(); bad[5] = np.nan
        code, text = _code(fe.means_points_set, bad, gy)
        assert code == INVALID and "grid point 5" in text
        bad = gy.copy(); bad[7] = np.inf
        assert _code(fe.means_points_set, gx, bad)[0] == INVALID
        bad = lon.copy(); bad[3] = np.nan
        assert _code(fe.means_points_set, gx, gy, rotation="north_east", gridLON=bad)[0] == INVALID
        p = _abi.MeansPoints(); p.G = -1
        assert fe.L.nxs_dyn_means_points_set(fe.h, C.byref(p)) == INVALID and b"G = -1" in fe.L.nxs_dyn_last_error(fe.h)
        # a refused set leaves the previous grid, and the handle works
        fe.means_points_update()
        ge, gn, _, _ = fe.means_points_get(apply_lsm=True)
        assert ge.shape == (3, gx.size) and gn.shape == (4, gx.size)
    finally:
        fe.close()
