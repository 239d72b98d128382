"""The coupler's outgoing fields on the device (nxs_dyn_cpl_out_*, nxs_dyn_fsd_diag_configure, nxs_gridmap_send_rows): M_cpl_out's second accumulator set,
D_dmax / D_dmean, the exchange grid's accumulators and the put (FE.cpp:8012-8052, 8226-8266, 7902-7951; gridoutput.cpp:387-415) against the fixtures of the real
contrib/bamg (tests/golden/bamg_grid_remap.npz, tests/golden/means_points.npz) and the restatement tests/cpl_out_ref.py.  Bit for bit, a NaN matching a NaN: there
is no tolerance anywhere in this feature."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from nextsim_amd import dynamics, forcing as F, interp, mesh as M

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import cases  # noqa: E402
import cpl_out_ref as CO  # noqa: E402
import grid_remap_ref as G  # noqa: E402
import make_means_points_golden as MG  # noqa: E402
import means_points_ref as P  # noqa: E402
from test_cpl_out_host_kernel import N_EL, awkward_grid, awkward_rows  # noqa: E402
from test_cpl_out_ref import fsd_case  # noqa: E402
from test_gpu_grid_remap import Dev, _case_map  # noqa: E402
from test_gpu_means import _handle, _ref_update, _same  # noqa: E402
from test_gpu_means_points import _global_mesh, _hip, _smooth_um, _state  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -4


def _code(fn, *a, **k):
    with pytest.raises(dynamics.NxsError) as e:
        fn(*a, **k)
    return e.value.code, str(e.value)


# ---- the elemental leg: nxs_gridmap_send_rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASES)
def test_send_rows_on_every_golden_case(name):
    """the real lists through nxs_gridmap_create; every build, the tile edge and the cap; awkward accumulators; the restatement AND mesh_to_grid transposed and added"""
    c, rg, gm = _case_map(name)
    lists, nels = CO.lists_of(c), c["tri"].shape[0]
    e = gm.export()
    assert np.array_equal(e["gridP"], c["gridP"]) and np.array_equal(e["tris"], c["tris"]) and G.same_bits(e["w"], c["w"])
    wet = np.zeros(lists["G"], bool)
    wet[lists["gridP"]] = True
    for nv in (1, 7):                                             # the real bamg's outputs on the wet rows, 0 on the dry ones
        got = gm.send_rows(c[f"m2g_in{nv}"])
        assert G.same_bits(got.T[wet] + 0., c[f"m2g_out{nv}"][wet] + 0.) and not got.T[~wet].any() and not np.signbit(got.T[~wet]).any()
    for n_el in N_EL:
        el, grid = awkward_rows(nels, n_el), awkward_grid(n_el, lists["G"])
        got = gm.send_rows(el, grid.copy())
        assert G.same_bits(got, CO.send_rows(lists, el, grid.copy())), (name, n_el)
        assert G.same_bits(got, grid + gm.mesh_to_grid(el, miss_val=0.).T), (name, n_el)
        once = gm.send_rows(el)
        assert G.same_bits(gm.send_rows(el, once.copy()), once + once), (name, n_el)          # a second put without a reset adds again
    # device pointers on both sides
    el, grid = awkward_rows(nels, 13), awkward_grid(13, lists["G"])
    din, dout = Dev(el.shape, el), Dev(grid.shape, grid)
    assert gm.send_rows(in_device=(din.p.value, 13), out_device=dout.p.value) is None
    assert G.same_bits(dout.get(), CO.send_rows(lists, el, grid.copy()))
    din.free(); dout.free()
    gm.close(); rg.close()


@pytest.mark.parametrize("n_local", [1, 255, 256, 257])
def test_send_rows_through_restricted_maps(n_local):
    """a partition's map gives the rank's partial sums; cells without a local triangle add 0."""
    c, rg, gm = _case_map("long_rows")
    nels = c["tri"].shape[0]
    order = np.argsort(-np.bincount(c["tris"], minlength=nels), kind="stable")[:n_local]      # triangles the lists name
    local = np.full(nels, -1, np.int32)
    local[np.sort(order)] = np.arange(n_local)
    r = gm.restrict(local, n_local)
    lists = CO.lists_of(dict(r.export(), cornerX=c["cornerX"], cornerY=c["cornerY"]))
    assert r.info()["nels"] == n_local and r.info()["wet"] >= 1
    for n_el in (5, 13):
        el, grid = awkward_rows(n_local, n_el) if n_local > 3 else np.full((n_local, n_el), -2.5), awkward_grid(n_el, lists["G"])
        assert G.same_bits(r.send_rows(el, grid.copy()), CO.send_rows(lists, el, grid.copy())), n_el
    r.close(); gm.close(); rg.close()


def synthetic_lists(nels, Gs, seed=17):
    """lists the kernel must simply apply: row lengths 0 .. 30, a cell that names one triangle twice, a dry first and a dry last cell (one wet cell when G == 1)"""
    rng = np.random.default_rng(seed + Gs)
    length = rng.integers(0, 31, Gs)
    if Gs >= 3:
        length[0] = length[-1] = 0
        length[1] = 30
        length[Gs // 2] = 4
    else:
        length[:] = 7
    gridP = np.flatnonzero(length > 0).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(length[gridP])]).astype(np.int32)
    tris = rng.integers(0, nels, off[-1]).astype(np.int32)
    twice = int(off[np.searchsorted(gridP, Gs // 2)]) if Gs >= 3 else 0
    tris[twice + 1] = tris[twice]                                 # one triangle twice in one row
    w = rng.uniform(0.1, 2., off[-1])
    side = rng.uniform(0.5, 2., Gs)
    x0 = np.arange(Gs) * 3.
    cornerX = np.stack([x0, x0 + side, x0 + side, x0], 1)
    cornerY = np.stack([np.zeros(Gs), np.zeros(Gs), side * 1.5, side * 1.5], 1)
    return {"gridP": gridP, "off": off, "tris": tris, "w": w, "cornerX": cornerX, "cornerY": cornerY, "nels": nels, "grid_size": Gs, "G": Gs}


@pytest.fixture(scope="module")
def holes_case():
    c = MG.means_points_case()
    c["z"] = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "means_points.npz")))
    return c


@pytest.mark.parametrize("Gs", [1, 255, 256, 257, 2173])
def test_send_rows_at_the_launch_edges(holes_case, Gs):
    nels = holes_case["tri"].shape[0]
    lists = synthetic_lists(nels, Gs)
    gm = interp.GridMap.import_(lists)
    for n_el in (1, 12, 13):
        el, grid = awkward_rows(nels, n_el), awkward_grid(n_el, Gs)
        got = gm.send_rows(el, grid.copy())
        assert G.same_bits(got, CO.send_rows(lists, el, grid.copy())), (Gs, n_el)
        assert G.same_bits(got, grid + gm.mesh_to_grid(el, miss_val=0.).T), (Gs, n_el)
    gm.close()


# ---- the whole put on the fixture's mesh ----------------------------------------------------------------------------------------------------------------------------
class Rig:
    """One handle on a mesh (x, y, tri 0-based, the first n_owned elements owned) with a configured coupler set whose accumulator rows the test seeds."""

    def __init__(self, x, y, tri, n_owned, UM, elemental, nodal):
        self.x, self.y, self.tri = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(tri)
        self.ne, self.nn, self.n_owned = self.tri.shape[0], self.x.size, n_owned
        lm = M.localize(_global_mesh(self.x, self.y, self.tri), 1)[0]
        assert np.array_equal(lm.indices.reshape(-1, 3) - 1, self.tri) and np.array_equal(lm.coord_x, self.x)
        self.lm = dataclasses.replace(lm, local_nelements=n_owned)
        self.fe = dynamics.FiniteElementDynamics(F.default_params(), device=0)
        self.fe.set_mesh(self.lm)
        self.fe.cpl_out_configure(elemental, nodal)
        self.move(UM)

    def move(self, UM):
        self.UM = UM
        self.fe.put_state(_state(self.lm, UM))

    def inject(self, el, nod):
        self.el, self.nod = el, nod
        _, _, de, dn = self.fe.cpl_out_get(want_host=False)
        for a, p in ((el, de), (nod, dn)):
            if a is not None and a.size:
                assert p and _hip().hipMemcpy(p, np.ascontiguousarray(a).ctypes.data, a.nbytes, 1) == 0

    def displaced(self):
        return self.x + self.UM[:self.nn], self.y + self.UM[self.nn:]


@pytest.mark.parametrize("rotation", ["north_east", "grid_theta", "none"])
def test_the_whole_put_on_the_fixtures_mesh(holes_case, rotation):
    """the fixture's points, both displaced meshes; the nodal columns against the real bamg's fixture, everything against the restatement"""
    c, z = holes_case, holes_case["z"]
    assert MG.ties(c) == (0, 0, 0)                                # no grid point on an edge, none left out: the fixture's generator asserts it too
    nodal = [v if isinstance(v, str) else v[0] for v in MG.NODAL]
    rig = Rig(c["x"], c["y"], c["tri"], c["n_owned"], c["UM1"], ("conc", "thick", "conc_cons"), nodal)
    fe = rig.fe
    lists = synthetic_lists(rig.ne, c["gx"].size)
    gm = interp.GridMap.import_(lists)
    try:
        rig.inject(c["el"], c["nod"])
        fe.cpl_out_attach_grid(gm, c["gx"], c["gy"], MG.MISS, rotation, gridLON=c["lon"], gridTheta=c["theta"], rotation_angle=MG.ROTATION_ANGLE, pairs=MG.PAIRS)
        cs, sn = P.cos_sin(rotation, MG.ROTATION_ANGLE, c["lon"], c["theta"])
        we, wn = np.zeros((3, c["gx"].size)), np.zeros((4, c["gx"].size))
        free = [0, 2, 3]                                          # the fixture's masked column is not this set's: it has no ice-mask rule
        for step, UM in enumerate((c["UM1"], c["UM2"])):
            rig.move(UM)
            ge, gn, de, dn = fe.cpl_out_put()
            xd, yd = rig.displaced()
            CO.put(we, wn, lists, c["el"], xd, yd, rig.tri, rig.n_owned, c["nod"], c["gx"], c["gy"], MG.PAIRS, cs, sn, MG.MISS)
            assert G.same_bits(ge, we) and P.equal(gn, wn), (rotation, step)
            key = {"north_east": ("gn1", "gn2"), "grid_theta": (None, "gn2_theta"), "none": (None, None)}[rotation][step]
            if key:
                assert P.equal(gn[free], z[key][free]), key
        # asynchronous: nothing copied, the device pointers are the resident rows
        _, _, de2, dn2 = fe.cpl_out_put(want_host=False)
        CO.put(we, wn, lists, c["el"], xd, yd, rig.tri, rig.n_owned, c["nod"], c["gx"], c["gy"], MG.PAIRS, cs, sn, MG.MISS)
        fe.synchronize()
        raw_e, raw_n = np.empty_like(we), np.empty_like(wn)
        assert (de2, dn2) == (de, dn) and de and dn
        assert _hip().hipMemcpy(raw_e.ctypes.data, de, raw_e.nbytes, 2) == 0 and _hip().hipMemcpy(raw_n.ctypes.data, dn, raw_n.nbytes, 2) == 0
        assert G.same_bits(raw_e, we) and P.equal(raw_n, wn)
        # reset_grid zeroes the grid rows alone
        fe.cpl_out_reset_grid()
        el_now, nod_now, _, _ = fe.cpl_out_get()
        assert G.same_bits(el_now, c["el"]) and P.equal(nod_now, c["nod"])
        ge, gn, _, _ = fe.cpl_out_put(reset=True)                  # FE.cpp:8262-8263 behind the copies
        assert G.same_bits(ge, CO.send_rows(lists, c["el"], np.zeros_like(we)))
        el_now, nod_now, _, _ = fe.cpl_out_get()
        assert not el_now.any() and not nod_now.any()
        ge, gn, _, _ = fe.cpl_out_put()
        assert not ge.any() and not gn.any()
    finally:
        fe.close(); gm.close()


def test_nodal_only_elemental_only_and_the_wave_models_list(holes_case):
    c = holes_case
    lists = synthetic_lists(c["tri"].shape[0], c["gx"].size)
    gm = interp.GridMap.import_(lists)
    rig = Rig(c["x"], c["y"], c["tri"], c["n_owned"], c["UM1"], (), ("VT_x", "VT_y"))
    fe = rig.fe
    try:
        xd, yd = rig.displaced()
        nod = np.ascontiguousarray(c["nod"][:, :2])
        rig.inject(None, nod)
        code, msg = _code(fe.cpl_out_attach_grid, gm)
        assert code == STATE and "no points" in msg
        fe.cpl_out_attach_grid(gm, c["gx"], c["gy"], MG.MISS, "north_east", gridLON=c["lon"], rotation_angle=MG.ROTATION_ANGLE, pairs=((0, 1),))
        ge, gn, de, dn = fe.cpl_out_put()
        cs, sn = P.cos_sin("north_east", MG.ROTATION_ANGLE, c["lon"], c["theta"])
        wn = CO.nodal_leg(np.zeros((2, c["gx"].size)), xd, yd, rig.tri, rig.n_owned, nod, c["gx"], c["gy"], ((0, 1),), cs, sn, MG.MISS)
        assert ge is None and not de and P.equal(gn, wn)
        assert not P.equal(gn, CO.nodal_leg(np.zeros((2, c["gx"].size)), xd, yd, rig.tri, rig.n_owned, nod, c["gx"], c["gy"], ((0, 1),), cs, sn, MG.MISS, drop=("no_proc_mask",)))
        # elemental only, no points: the grid is another set of lists of the same size, so the (re-made) accumulators start from zero
        fe.cpl_out_configure(("damage", "ridge_ratio", "conc_cons", "conc", "thick"), ())
        el = awkward_rows(rig.ne, 5)
        rig.inject(el, None)
        fe.cpl_out_attach_grid(gm)
        ge, gn, de, dn = fe.cpl_out_put()
        assert gn is None and not dn and G.same_bits(ge, CO.send_rows(lists, el, np.zeros((5, c["gx"].size))))
        # the wave model's list, without points and without bins attached (M_num_fsd_bins == 0: dmax / dmean accumulate 0)
        fe.cpl_out_configure(("conc", "thick", "dmax", "dmean"), ())
        fe.cpl_out_attach_grid(gm)
        fe.cpl_out_update(0.5)
        st = _state(rig.lm, rig.UM)
        el, _, _, _ = fe.cpl_out_get()
        n = rig.n_owned
        D_conc = st["conc"] + st["conc_young"] if F.default_params().ice_cat_type == 1 else st["conc"]
        assert G.same_bits(el[:n, 0], D_conc[:n] * 0.5) and not el[:, 2:].any() and not el[n:].any()
        ge, _, _, _ = fe.cpl_out_put()
        assert G.same_bits(ge, CO.send_rows(lists, el, np.zeros((4, c["gx"].size))))
    finally:
        fe.close(); gm.close()


# ---- the two sets ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_moorings_and_coupler_do_not_see_each_other():
    fe, lm, p, f = _handle("toy")
    moor = (("conc_cons", "damage", "sigma_11"), ("VT_x", "VT_y", "wind_x"))
    cpl = (("ridge_ratio", "conc", "thick", "conc_cons", "sigma_22"), ("VT_y",))
    both = CO.TwoSets(lm.num_nodes, lm.num_elements, lm.local_nelements, p.ice_cat_type == 1)
    fe.means_configure(*moor); both.configure("moorings", *moor)
    fe.cpl_out_configure(*cpl); both.configure("cpl_out", *cpl)
    try:
        for step in range(3):
            fe.step()
            fe.means_update(0.25); fe.cpl_out_update(1. if step == 0 else 1. / 3.)             # (pcpt == 0) ? 1 : dtime_step / cpl_time_step
            for which, tf in (("moorings", 0.25), ("cpl_out", 1. if step == 0 else 1. / 3.)):
                _ref_update(both.sets[which], fe, f, tf)

        def check(what):
            el, nod, _, _ = fe.means_get()
            cel, cnod, _, _ = fe.cpl_out_get()
            for got, want in zip((el, nod, cel, cnod), both.rows("moorings") + both.rows("cpl_out")):
                assert _same(got, want), what
        check("three steps")
        assert both.sets["cpl_out"].el.any() and both.sets["moorings"].nod.any()
        fe.cpl_out_reset(); both.reset("cpl_out"); check("coupler reset")
        fe.cpl_out_update(0.5); _ref_update(both.sets["cpl_out"], fe, f, 0.5)
        fe.means_reset(); both.reset("moorings"); check("moorings reset")
        fe.means_update(2.); _ref_update(both.sets["moorings"], fe, f, 2.)
        # configuring one again, or dropping it, leaves the other's bits alone
        el0, nod0, _, _ = fe.means_get()
        fe.cpl_out_configure(("damage",), ())
        assert not fe.cpl_out_get()[0].any()
        fe.cpl_out_configure((), ())
        code, msg = _code(fe.cpl_out_update, 1.)
        assert code == STATE and "cpl_out_update" in msg and "no variable is configured" in msg
        el1, nod1, _, _ = fe.means_get()
        assert _same(el1, el0) and _same(nod1, nod0)
        fe.cpl_out_configure(*cpl); both.configure("cpl_out", *cpl)
        fe.cpl_out_update(1.); _ref_update(both.sets["cpl_out"], fe, f, 1.)
        cel0, cnod0, _, _ = fe.cpl_out_get()
        fe.means_configure((), ())
        cel1, cnod1, _, _ = fe.cpl_out_get()
        assert _same(cel1, cel0) and _same(cnod1, cnod0) and _same(cel1, both.rows("cpl_out")[0])
    finally:
        fe.close()


def test_the_three_output_grids_of_one_handle_do_not_see_each_other():
    """A loaded grid of 7 points, a regular grid of 3 x 5 and the exchange grid of the smallest golden case on ONE handle, each accumulated once from seeded mesh
    rows: other Moorings lists re-make both Moorings grids zeroed and leave the coupler's rows alone, other coupler lists leave both Moorings grids alone.  Bit for bit."""
    fe, lm, p, f = _handle("toy")
    c = G.case(min(G.CASES, key=lambda name: G.case(name)["gridX"].size))
    lists = dict(CO.lists_of(c), nels=lm.num_elements)            # the case's lists read as lists on this mesh: every triangle they name exists here
    lists["grid_size"] = Gc = lists["G"]
    assert len({7, 3 * 5, Gc}) == 3 and c["gridP"].size and c["tris"].max() < lm.num_elements
    gm = interp.GridMap.import_(lists)
    xm, ym = 0.5 * (lm.coord_x.min() + lm.coord_x.max()), 0.5 * (lm.coord_y.min() + lm.coord_y.max())
    dx, dy = 0.1 * np.ptp(lm.coord_x), 0.1 * np.ptp(lm.coord_y)   # all three grids lie well inside the mesh

    def raw(ptr, shape):
        a = np.empty(shape)
        assert ptr and _hip().hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
        return a

    def seed(get, n_el, n_nod):
        """both mesh accumulators of a set ([Ne, n_el], [Nn, n_nod]) filled with values in [1, 2): whatever a grid gathers from them inside the mesh is not zero"""
        fe.synchronize()
        _, _, de, dn = get(want_host=False)
        rng = np.random.default_rng(n_el + 10 * n_nod)
        for ptr, count in ((de, lm.num_elements * n_el), (dn, lm.num_nodes * n_nod)):
            a = rng.uniform(1., 2., count)
            assert not count or (ptr and _hip().hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0)

    def moorings(n_el, n_nod):
        out = fe.means_points_get()[:2] + fe.means_regular_get()[:2]
        for a, shape in zip(out, ((n_el, 7), (n_nod, 7), (n_el, 15), (n_nod, 15))):
            assert (a is None and shape[0] == 0) or a.shape == shape, shape
        return out
    try:
        fe.means_configure(("conc", "thick"), ("VT_x", "VT_y"))
        fe.cpl_out_configure(("conc", "damage", "thick"), ("VT_x", "VT_y"))
        fe.means_points_set(xm + dx * np.linspace(-3., 3., 7), ym + dy * np.sin(np.arange(7.)))       # (no pairs: they would not outlive the nodal list)
        fe.means_regular_set(xm - dx, ym + 2. * dy, dy, ncols=3, nrows=5)
        fe.cpl_out_attach_grid(gm, xm + dx * np.cos(np.arange(Gc) + 1.), ym + dy * np.sin(np.arange(Gc) + 1.), pairs=((0, 1),))
        seed(fe.means_get, 2, 2); seed(fe.cpl_out_get, 3, 2)
        fe.means_points_update(); fe.means_regular_update()
        ce, cn, de, dn = fe.cpl_out_put()
        assert ce.shape == (3, Gc) and cn.shape == (2, Gc) and ce.any() and cn.any()
        assert all(a.any() for a in moorings(2, 2))
        # (2 elemental, 2 nodal) -> (1, 0): both Moorings grids come back zeroed at the new sizes, the coupler's rows keep their bits
        fe.means_configure(("conc",), ())
        pe, pn, re_, rn = moorings(1, 0)
        assert not pe.any() and not re_.any() and pn is None and rn is None
        fe.synchronize()
        assert _same(raw(de, ce.shape), ce) and _same(raw(dn, cn.shape), cn)
        # ... and accumulated at the new sizes they keep theirs when the coupler's lists change
        seed(fe.means_get, 1, 0)
        fe.means_points_update(); fe.means_regular_update()
        pe, _, re_, _ = moorings(1, 0)
        assert pe.any() and re_.any()
        fe.cpl_out_configure(("conc",), ("VT_x", "VT_y", "wind_x"))
        pe1, _, re1, _ = moorings(1, 0)
        assert _same(pe1, pe) and _same(re1, re_)
        fe.cpl_out_attach_grid(gm, xm + dx * np.cos(np.arange(Gc) + 1.), ym + dy * np.sin(np.arange(Gc) + 1.), pairs=((0, 1),))
        ce, cn, _, _ = fe.cpl_out_put()                            # (its mesh rows were re-made zeroed: the re-made grid rows hold what zeros add up to)
        assert ce.shape == (1, Gc) and cn.shape == (3, Gc) and not ce.any()
        pe1, _, re1, _ = moorings(1, 0)
        assert _same(pe1, pe) and _same(re1, re_)
    finally:
        fe.close(); gm.close()


# ---- dmax / dmean -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("nb", [1, 2, 12, 16])
def test_dmax_dmean_on_the_device(nb, young):
    """every branch of FE.cpp:7902-7951 on the elements 250 .. 258, so that the block edges 255 / 256 / 257 carry such elements; both sets accept the ids"""
    gm = cases.global_mesh("toy")
    lm = M.localize(gm, 1)[0]
    p = F.default_params()
    p.ice_cat_type = 1 if young else 0
    Ne, at = lm.num_elements, 250
    st = _state(lm, np.zeros(2 * lm.num_nodes))
    st["conc"][at] = 0.; st["conc"][at + 1:at + 4] = st["conc"][at + 1]
    st["conc_young"] = 0.3 * st["conc_young"]
    st["conc_young"][at] = 0.; st["conc_young"][at + 1:at + 4] = st["conc_young"][at + 1]
    D_conc = st["conc"] + st["conc_young"] if young else st["conc"].copy()
    mech, D_conc, up, centres = fsd_case(nb, at=at, negative=False, D_conc=D_conc)
    tables = dynamics.fsd_bins("constant_size", nb, 10., 20.)
    assert np.array_equal(tables["bin_up_limits"], up) and np.array_equal(tables["bin_centres"], centres)
    fe = dynamics.FiniteElementDynamics(p, device=0)
    try:
        fe.set_mesh(lm); fe.put_state(st)
        lst = ("dmax", "conc", "dmean")
        fe.cpl_out_configure(lst, ()); fe.means_configure(("dmean", "dmax"), ())
        fe.put_coupled(conc_fsd=mech)
        code, msg = _code(fe.cpl_out_update, 1.)
        assert code == STATE and "dmax" in msg and "M_conc_mech_fsd" in msg and "cpl_out_update" in msg
        fe.fsd_put(conc_mech_fsd=mech)
        code, msg = _code(fe.cpl_out_update, 1.)
        assert code == STATE and "dmax" in msg and "nxs_dyn_fsd_configure" in msg
        fe.fsd_configure(tables)
        code, msg = _code(fe.means_update, 1.)
        assert code == STATE and "dmean" in msg and "nxs_dyn_fsd_diag_configure" in msg and "means_update" in msg
        n = lm.local_nelements
        acc = np.zeros((Ne, 3)); macc = np.zeros((Ne, 2))
        for opts, tf in ((CO.DEFAULTS, 1.), ({"dmax_c_threshold": 0.25, "fsd_unbroken_floe_size": 300., "fsd_min_floe_size": 35.}, 1. / 3.)):
            fe.fsd_diag_configure(**opts)
            fe.cpl_out_update(tf); fe.means_update(tf)
            dmax, dmean = CO.fsd_diag(mech, D_conc, up, centres, **opts)
            CO.fsd_means(acc[:, 0], acc[:, 2], dmax, dmean, n, tf)
            CO.fsd_means(macc[:, 1], macc[:, 0], dmax, dmean, n, tf)
            acc[:n, 1] += D_conc[:n] * tf
        el, _, _, _ = fe.cpl_out_get()
        mel, _, _, _ = fe.means_get()
        assert G.same_bits(el, acc) and G.same_bits(mel, macc)
        wrong = CO.fsd_diag(mech, D_conc, up, centres, drop=("strict_threshold",))
        assert not G.same_bits(wrong[0], CO.fsd_diag(mech, D_conc, up, centres)[0])
        code, msg = _code(fe.fsd_diag_configure, float("nan"), 1000., 10.)
        assert code == INVALID and "finite" in msg
    finally:
        fe.close()


# ---- life cycle and refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_update_put_regrid_attach_update_put_and_every_refusal():
    x, y, tri, ng = cases.rect_mesh(25, 1)
    x, y, tri = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64), np.ascontiguousarray(tri, np.int32)
    um = _smooth_um(x, y, tri)
    gx, gy, lon, theta = MG.curvilinear_grid(x, y, 17, 15, seed=8)
    Gs = gx.size
    fe0 = dynamics.FiniteElementDynamics(F.default_params(), device=0)
    code, msg = _code(fe0.cpl_out_update, 1.)
    assert code == STATE and "set_mesh" in msg
    fe0.close()
    rig = Rig(x, y, tri, tri.shape[0], um, ("conc_cons", "damage"), ("VT_x", "VT_y"))
    fe = rig.fe
    lists = synthetic_lists(rig.ne, Gs)
    gm = interp.GridMap.import_(lists)
    other = interp.GridMap.import_(synthetic_lists(rig.ne + 1, Gs))
    small = interp.GridMap.import_(synthetic_lists(rig.ne, 256))
    try:
        assert P.ties(*rig.displaced(), rig.tri, gx, gy) == 0
        # refusals, by code and by the name in the message
        code, msg = _code(fe.cpl_out_configure, (("conc_cons", True), "ice_mask"), ())
        assert code == INVALID and "mask" in msg and "cpl_out_configure" in msg
        code, msg = _code(fe.cpl_out_configure, (200,), ())
        assert code == INVALID and "elemental_ids[0] = 200" in msg
        code, msg = _code(fe.cpl_out_configure, (), ("conc",))
        assert code == INVALID and "nodal_ids[0]" in msg
        code, msg = _code(fe.cpl_out_put)
        assert code == STATE and "no exchange grid" in msg
        code, msg = _code(fe.cpl_out_reset_grid)
        assert code == STATE and "no exchange grid" in msg
        code, msg = _code(fe.cpl_out_attach_grid, other, gx, gy)
        assert code == STATE and "elements" in msg
        code, msg = _code(fe.cpl_out_attach_grid, small, gx, gy)
        assert Gs == 255 and code == INVALID and "256 cells" in msg and "the points are 255" in msg
        code, msg = _code(fe.cpl_out_attach_grid, gm, gx, gy, MG.MISS, "north_east")
        assert code == INVALID and "gridLON" in msg and "cpl_out_attach_grid" in msg
        code, msg = _code(fe.cpl_out_attach_grid, gm, gx, gy, MG.MISS, "none", pairs=((0, 2),))
        assert code == INVALID and "pair 0" in msg
        fe.cpl_out_configure(("conc_cons", "damage"), ("tauwix",))
        code, msg = _code(fe.cpl_out_update, 1.)
        assert code == STATE and "wave stress" in msg and "cpl_out_update" in msg
        fe.cpl_out_configure(("conc_cons", "sst"), ("taux",))
        code, msg = _code(fe.cpl_out_update, 1.)
        assert code == STATE and "D_tau_ow" in msg and "cpl_out_update" in msg
        fe.cpl_out_configure(("conc_cons", "sst"), ())
        code, msg = _code(fe.cpl_out_update, 1.)
        assert code == STATE and "sst" in msg and "cpl_out_update" in msg
        fe.cpl_out_configure(("conc_cons", "damage"), ("VT_x", "VT_y"))
        fe.cpl_out_attach_grid(gm, gx, gy, MG.MISS, "grid_theta", gridTheta=theta, rotation_angle=MG.ROTATION_ANGLE, pairs=((0, 1),))
        code, msg = _code(fe.cpl_out_put, want_host=False, reset=True)
        assert code == INVALID and "NXS_CPL_OUT_RESET" in msg
        # update -> put
        cs, sn = P.cos_sin("grid_theta", MG.ROTATION_ANGLE, lon, theta)
        st = _state(rig.lm, um)
        fe.cpl_out_update(0.5)
        el, nod, _, _ = fe.cpl_out_get()
        assert G.same_bits(el[:, 0], st["conc"] * 0.5) and G.same_bits(nod[:, 1], st["VT"][rig.nn:] * 0.5)
        we, wn = np.zeros((2, Gs)), np.zeros((2, Gs))
        ge, gn, _, _ = fe.cpl_out_put()                           # (FE.cpp:8014: the put in front of a regrid)
        CO.put(we, wn, lists, el, *rig.displaced(), rig.tri, rig.n_owned, nod, gx, gy, ((0, 1),), cs, sn, MG.MISS)
        assert G.same_bits(ge, we) and P.equal(gn, wn) and ge.any() and gn.any()
        # an identity regrid: the mesh rows restart, the map is gone with the old mesh, the grid rows carry over
        prev = np.arange(1, rig.nn + 1, dtype=np.float64)
        fe.regrid(rig.lm, prev, ng, {k: st[k] for k in dynamics.REGRID_INPUTS}, (), moved=(rig.lm.coord_x, rig.lm.coord_y))
        el0, nod0, _, _ = fe.cpl_out_get()
        assert not el0.any() and not nod0.any()
        code, msg = _code(fe.cpl_out_put)
        assert code == STATE and "no exchange grid" in msg and "nxs_dyn_regrid" in msg
        fe.cpl_out_attach_grid(gm, gx, gy, MG.MISS, "grid_theta", gridTheta=theta, rotation_angle=MG.ROTATION_ANGLE, pairs=((0, 1),))
        rig.move(0.5 * um)
        assert P.ties(*rig.displaced(), rig.tri, gx, gy) == 0
        fe.cpl_out_update(1.)
        el, nod, _, _ = fe.cpl_out_get()
        ge, gn, _, _ = fe.cpl_out_put()
        CO.put(we, wn, lists, el, *rig.displaced(), rig.tri, rig.n_owned, nod, gx, gy, ((0, 1),), cs, sn, MG.MISS)
        assert G.same_bits(ge, we) and P.equal(gn, wn)
        # set_mesh as well: configuration and grid rows survive, the accumulators restart zeroed
        fe.set_mesh(rig.lm); rig.move(um)
        assert not fe.cpl_out_get()[0].any()
        fe.cpl_out_attach_grid(gm, gx, gy, MG.MISS, "grid_theta", gridTheta=theta, rotation_angle=MG.ROTATION_ANGLE, pairs=((0, 1),))
        ge, gn, _, _ = fe.cpl_out_put(reset=True)
        assert G.same_bits(ge, we) and P.equal(gn, wn)
        ge, gn, _, _ = fe.cpl_out_put()
        assert not ge.any() and not gn.any()
    finally:
        fe.close(); gm.close(); other.close(); small.close()
