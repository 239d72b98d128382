"""nxs_dyn_regrid on the GPU: FiniteElement::interpFields + assignVariables on the live handle against the host chain of tests/regrid_ref.py
(collectVariables -> ConservativeRemappingMeshToMesh -> redistributeVariables, gatherFieldsNode -> InterpFromMeshToMesh2dx -> scatterFieldsNode).

Expected agreement: BITWISE, every variable.  What the new kernels add to the two interpolations (already bit-identical to the real bamg) is one IEEE
multiply, divide, square root, max or min per value on doubles, compiled without contraction; the enthalpy inverse's square root is the compiler's
correctly rounded one, so it gets no bound of its own."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import regrid_ref as R
from nextsim_amd import _abi, dynamics, forcing as F, mesh as M
from nextsim_amd.interp import ConservativeRemappingMeshToMesh, InterpFromMeshToMesh2dx
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bamg_regrid.npz")
MU = 0.055


def _eq(a, b):
    """bitwise, NaN == NaN"""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _global_mesh(x, y, tri, ngeom):
    on_b = np.zeros(x.size, bool); on_b[:ngeom] = True
    return M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=on_b,
                        neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="regrid")


def _remap(index_old, xo, yo, index_new, xn, yn, prev, ngeom, rows):
    return ConservativeRemappingMeshToMesh(rows, index_old, xo, yo, index_new, xn, yn, prev, ngeom)


def _interp(index_old, xo, yo, nod, xn, yn):
    return InterpFromMeshToMesh2dx(index_old, xo, yo, nod, xn, yn, False)


@functools.lru_cache(maxsize=None)
def _hip():
    """The HIP runtime libnxsdyn.so itself is linked against (one runtime in the process): plain device buffers for the extras passed as device pointers."""
    out = subprocess.check_output(["readelf", "-d", dynamics._LIB_PATH], text=True)
    name = [n for n in re.findall(r"NEEDED.*\[(.*)\]", out) if "amdhip64" in n][0]
    dynamics.load_library()
    hip = C.CDLL(name)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _dev_put(a):
    p = C.c_void_p()
    assert _hip().hipMalloc(C.byref(p), a.nbytes) == 0
    assert _hip().hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
    return p.value


def _dev_get(ptr, n):
    out = np.empty(n)
    assert _hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(old x, y, tri0, new x, y, tri0, previous_numbering, n_geom).  'golden': the real remesher's output; 'rect': cases.adapted_mesh on a box the 'arctic'
    fields put an ice edge through -- 1246 -> 1308 triangles, 672 -> 703 nodes: all different, none a multiple of 64, five / six blocks of 256."""
    if name == "golden":
        d = np.load(GOLDEN)
        return d["x_old"], d["y_old"], d["tri_old"], d["x_new"], d["y_new"], d["tri_new"], d["prev"], int(d["ngeom"])
    x, y, tri, ng = cases.rect_mesh(24, 1, x0=300e3, y0=0.)
    xn, yn, tn, prev = cases.adapted_mesh(x, y, tri, ng, 3)
    sizes = (tri.shape[0], tn.shape[0], x.size, xn.size)
    assert len(set(sizes)) == 4 and all(s % 64 for s in sizes)
    return x, y, tri, xn, yn, tn, prev, ng


def _fields(gm, young):
    p = F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)
    p, C_fix, C_alea = F.scale_params_to_mesh(p, gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    if not (g["thick"] == 0.).any():
        # the golden box lies where the 'arctic' fields are all ice: an ice-free corner and a fringe of young ice, so that no_old_ice and the cap have elements
        cx = gm.x[gm.tri].mean(1)
        ow = cx > gm.x.min() + 0.8 * np.ptp(gm.x); fringe = ~ow & (cx > gm.x.min() + 0.7 * np.ptp(gm.x))
        for k in ("conc", "thick", "snow_thick", "conc_myi", "thick_myi"):
            g[k][ow] = 0.
        g["conc"][fringe] = 0.6; g["conc_young"][fringe] = 0.3; g["h_young"][fringe] = 0.05
    lm = M.localize(gm, 1)[0]
    assert np.array_equal(lm.node_gid, np.arange(gm.num_nodes)) and np.array_equal(lm.elem_gid, np.arange(gm.num_elements))
    return p, lm, F.localize_fields(g, lm, gm.num_nodes)


def _extras(rng, st, Ne):
    """One variable of every kind (FE.cpp:2136-2147): `none` with a minimum above some of its values, conc, thick, two enthalpy layers flagged M_tice."""
    tice = lambda: np.where(st["thick"] > 0, rng.uniform(-30., -0.5, Ne), -MU * R.SI)   # noqa: E731
    return [dict(old=rng.uniform(-2., 30., Ne), transformation="none", min=1.5),              # an M_sst-like variable, clipped from below
            dict(old=rng.uniform(0., 1., Ne), transformation="conc", min=0., max=1.),         # a pond fraction per ice area
            dict(old=tice(), transformation="enthalpy", max=0., is_tice=True),                # M_tice[1]
            dict(old=rng.uniform(0., 40., Ne), transformation="thick", min=0.),               # an age per volume
            dict(old=tice(), transformation="enthalpy", max=0., is_tice=True)]                # M_tice[2]


@functools.lru_cache(maxsize=None)
def _run(pair, young=True, coupled=False, device_extra=False, go_on=False):
    """3 steps on the old mesh, then nxs_dyn_regrid and the host chain on the same inputs; go_on: 5 more steps on both sides."""
    xo, yo, to, xn, yn, tn, prev, ng = _pair(pair)
    gm, gm2 = _global_mesh(xo, yo, to, ng), _global_mesh(xn, yn, tn, ng)
    p, lm, f = _fields(gm, young)
    _, lm2, f2 = _fields(gm2, young)
    rng = np.random.default_rng(11)
    Ne, Nn, Ne2 = lm.num_elements, lm.num_nodes, lm2.num_elements
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    if coupled:
        rc = np.random.default_rng(12)      # (a generator of its own: the extras below are the same with and without the coupled columns)
        fe.put_coupled(cum_damage=rc.uniform(0., 0.2, Ne), conc_fsd=np.ascontiguousarray(rc.dirichlet([1., 1., 1.], Ne).T * f["conc"]))
    for _ in range(3):
        fe.step()
    fe.synchronize()
    st = fe.get_state()
    cp = fe.get_coupled(True, 3) if coupled else None
    assert np.abs(st["UM"]).max() > 0. and np.abs(st["UT"]).max() > 0. and np.abs(st["sigma0"]).max() > 0.
    xm, ym = lm.coord_x + st["UM"][:Nn], lm.coord_y + st["UM"][Nn:]
    extras = _extras(rng, st, Ne)
    assert (extras[0]["old"] < 1.5).any() and (st["thick"] == 0.).any()
    # ---- the host chain
    ref, ref_extras, nb_var = R.chain(st, (to, xm, ym), (tn, xn, yn), prev, ng, young, _remap, _interp, extras, cp, MU)
    # ---- the library
    given = [dict(x) for x in extras]
    dev = None
    if device_extra:     # the `thick` variable lives on the device on both meshes
        dev = (_dev_put(np.ascontiguousarray(extras[3]["old"])), _dev_put(np.zeros(Ne2)))
        given[3]["old"], given[3]["new"] = dev
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    info = fe.regrid(lm2, prev, ng, inputs, given, moved=(xm, ym), freezingpoint_mu=MU)
    got = fe.get_state()
    got_extras = [x["new"] for x in given]
    if dev:
        got_extras[3] = _dev_get(dev[1], Ne2)
        for q in dev:
            _hip().hipFree(q)
    out = dict(ref=ref, got=got, ref_extras=ref_extras, got_extras=got_extras, info=info, nb_var=nb_var, lm2=lm2, f2=f2, p=p, diag=fe.get_diag(),
               got_coupled=fe.get_coupled(True, 3) if coupled else None)
    if go_on:
        fe.set_forcing(f2)
        for _ in range(5):
            fe.step()
        fe.synchronize()
        out["checks"] = (fe.checkRegridding(), fe.checkFieldsFast())
        out["after"] = fe.get_state()
        fresh = dynamics.FiniteElementDynamics(p)
        fresh.set_mesh(lm2); fresh.put_state(dict(ref, **inputs)); fresh.set_forcing(f2)
        for _ in range(5):
            fresh.step()
        fresh.synchronize()
        out["fresh_checks"] = (fresh.checkRegridding(), fresh.checkFieldsFast())
        out["fresh_after"] = fresh.get_state()
        fresh.close()
    fe.close()
    return out


def _assert_state(r):
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
        assert _eq(r["got"][k], r["ref"][k]), k
    for i, (a, b) in enumerate(zip(r["got_extras"], r["ref_extras"])):
        assert _eq(a, b), f"extra {i}"
    n2 = 2 * r["lm2"].num_nodes
    assert _eq(r["got"]["UM"], np.zeros(n2)) and _eq(r["got"]["UT"], np.zeros(n2))
    assert _eq(r["diag"]["D_tau_a"], np.zeros(n2)) and _eq(r["diag"]["D_tau_w"], np.zeros(n2))     # scatterFieldsNode, FE.cpp:3277-3278
    assert r["info"]["num_failed"] == 0 and r["info"]["nb_var_element"] == r["nb_var"]


# ---- 2. identity regrid: the rules of redistributeVariables bite, the interpolations change nothing ----------------------------------------

@pytest.mark.parametrize("young", [True, False])
def test_identity_regrid(young):
    x, y, tri, ng = cases.rect_mesh(24, 1)
    gm = _global_mesh(x, y, tri, ng)
    p, lm, f = _fields(gm, young)
    Ne, Nn = lm.num_elements, lm.num_nodes
    rng = np.random.default_rng(5)
    f = {k: v.copy() for k, v in f.items()}
    f["conc"][:] = 0.9; f["thick"][:] = 1.2; f["conc_young"][:] = 0.05; f["h_young"][:] = 0.01
    sel = rng.permutation(Ne)
    f["damage"][:] = rng.uniform(0., 0.9, Ne); f["damage"][sel[:50]] = 1.0                       # capped at 1 - 1e-10
    f["conc_young"][sel[50:120]] = 0.3                                                           # conc + conc_young = 1.2
    ow = sel[120:200]
    f["conc"][ow] = 0.; f["thick"][ow] = 0.                                                      # no old ice
    for k in ("sigma0", "sigma1", "sigma2"):
        f[k][:] = rng.normal(0., 2e3, Ne)                                                        # both signs, unbounded
    f["ridge_ratio"][:] = rng.uniform(0., 1., Ne)
    f["VT"][:] = rng.normal(0., 0.1, 2 * Nn); f["UM"][:] = 0.; f["UT"][:] = rng.normal(0., 50., 2 * Nn)
    extras = [dict(old=np.where(f["thick"] > 0, rng.uniform(-30., -0.5, Ne), -1.), transformation="enthalpy", max=0., is_tice=True),
              dict(old=rng.uniform(0., 1., Ne), transformation="conc", min=0., max=1.)]
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    st = fe.get_state()
    prev = np.arange(1, Nn + 1, dtype=np.float64)
    ref, ref_extras, nb_var = R.chain(st, (tri, x, y), (tri, x, y), prev, ng, young, _remap, _interp, extras, None, MU)
    given = [dict(e) for e in extras]
    info = fe.regrid(lm, prev, ng, {k: f[k] for k in dynamics.REGRID_INPUTS}, given, moved=(x, y), freezingpoint_mu=MU)
    got = fe.get_state()
    fe.close()
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
        assert _eq(got[k], ref[k]), k
    for i in range(2):
        assert _eq(given[i]["new"], ref_extras[i]), i
    assert info["num_failed"] == 0 and info["nb_var_element"] == nb_var == 15
    assert got["damage"].max() == 1. - 1e-10 and (got["damage"] == 1. - 1e-10).sum() == 50
    if young:                                                                                    # the cap of FE.cpp:2253-2256 ...
        assert (got["conc"] + got["conc_young"]).max() <= 1. and _eq(got["conc_young"][sel[50:120]], 1. - got["conc"][sel[50:120]])
    else:                                                                                        # ... is the young-ice category's alone
        assert got["conc_young"][sel[50:120]].min() > 0.29 and (got["conc"] + got["conc_young"]).max() > 1.
    assert _eq(given[0]["new"][ow], np.full(ow.size, -MU * R.SI))                                # no_old_ice: M_tice = -mu * si
    assert _eq(got["UM"], np.zeros(2 * Nn)) and _eq(got["UT"], np.zeros(2 * Nn))
    inside = np.concatenate([np.arange(ng, Nn), Nn + np.arange(ng, Nn)])
    assert _eq(got["VT"][inside], st["VT"][inside])                                              # P1 interpolation at a mesh's own nodes
    for k in ("sigma0", "sigma1", "sigma2"):                                                     # one old triangle each: in * area * (1 / area)
        assert np.allclose(got[k], st[k], rtol=1e-15, atol=0.) and (got[k] < 0).any() and (got[k] > 0).any(), k


# ---- 3. a real regrid ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["golden", "rect"])
def test_regrid_from_fixtures(pair):
    r = _run(pair, True, False, pair == "rect", pair == "golden")
    _assert_state(r)
    assert r["nb_var"] == 13 + 5
    got, ex = r["got"], r["got_extras"]
    assert (got["thick"] == 0.).any() and _eq(ex[2][got["thick"] <= 0.], np.full((got["thick"] <= 0.).sum(), -MU * R.SI))
    assert ex[0].min() == 1.5 and (got["conc"] + got["conc_young"]).max() <= 1. and got["damage"].max() <= 1. - 1e-10
    assert not _eq(got["conc"], np.ones_like(got["conc"])) and np.abs(got["VT"]).max() > 0.


@pytest.mark.skipif(O.bamg_shim() is None, reason="oracle/_ref (the real contrib/bamg) not present")
def test_regrid_against_the_real_bamg():
    """The same chain with the reference's own ConservativeRemappingMeshToMesh and InterpFromMeshToMesh2dx in the place of the repository's."""
    r = _run("golden", True, False, False, True)
    xo, yo, to, xn, yn, tn, prev, ng = _pair("golden")
    # the inputs of the chain are not kept by _run: rebuilt from the same seeds
    gm = _global_mesh(xo, yo, to, ng)
    p, lm, f = _fields(gm, True)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    for _ in range(3):
        fe.step()
    fe.synchronize()
    st = fe.get_state()
    fe.close()
    Nn = lm.num_nodes
    xm, ym = lm.coord_x + st["UM"][:Nn], lm.coord_y + st["UM"][Nn:]
    extras = _extras(np.random.default_rng(11), st, lm.num_elements)
    ref, ref_extras, _ = R.chain(st, (to, xm, ym), (tn, xn, yn), prev, ng, True,
                                 lambda io, a, b, inw, c, d, pn, n, rows: O.bamg_conservative_remap(io, a, b, inw, c, d, pn, n, rows),
                                 lambda io, a, b, nod, c, d: O.bamg_interp_mesh_to_mesh(io, a, b, nod, c, d, False), extras, None, MU)
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
        assert _eq(r["got"][k], ref[k]), k
    for i, (a, b) in enumerate(zip(r["got_extras"], ref_extras)):
        assert _eq(a, b), f"extra {i}"


def test_rows_wider_than_the_staging_tile():
    """More than 31 columns: the kernels walk their rows in global memory instead of staging them through LDS (NXS_REGRID_STAGE_MAX) -- the other path, same bits."""
    xo, yo, to, xn, yn, tn, prev, ng = _pair("rect")
    p, lm, f = _fields(_global_mesh(xo, yo, to, ng), True)
    _, lm2, f2 = _fields(_global_mesh(xn, yn, tn, ng), True)
    rng = np.random.default_rng(21)
    Ne = lm.num_elements
    kinds = ("none", "conc", "thick", "enthalpy")
    extras = [dict(old=rng.uniform(-20., -1., Ne), transformation=kinds[i % 4], max=0., is_tice=i % 4 == 3) for i in range(19)]   # 13 + 19 = 32 columns
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    st = fe.get_state()
    ref, ref_extras, nb_var = R.chain(st, (to, xo, yo), (tn, xn, yn), prev, ng, True, _remap, _interp, extras, None, MU)
    given = [dict(e) for e in extras]
    info = fe.regrid(lm2, prev, ng, {k: f2[k] for k in dynamics.REGRID_INPUTS}, given, moved=(xo, yo), freezingpoint_mu=MU)
    got = fe.get_state()
    fe.close()
    assert info["nb_var_element"] == nb_var == 32 and info["num_failed"] == 0
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
        assert _eq(got[k], ref[k]), k
    for i in range(19):
        assert _eq(given[i]["new"], ref_extras[i]), i


# ---- 4. the coupled build's columns ride along ----------------------------------------------------------------------------------------------

def test_coupled_columns():
    with_c, without = _run("rect", True, True, False, False), _run("rect", True, False, True, False)
    _assert_state(with_c)
    assert with_c["nb_var"] == 13 + 1 + 3 + 5 and without["nb_var"] == 13 + 5
    assert _eq(with_c["got_coupled"]["cum_damage"], with_c["ref"]["cum_damage"])
    assert _eq(with_c["got_coupled"]["conc_fsd"], np.stack([with_c["ref"][f"conc_fsd{b}"] for b in range(3)]))
    assert with_c["got_coupled"]["cum_damage"].min() >= 0. and with_c["got_coupled"]["conc_fsd"].max() <= 1.
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:      # more columns, the same rows: cum_damage is an output of the sub-steps, not an input
        assert _eq(with_c["got"][k], without["got"][k]), k
    for a, b in zip(with_c["got_extras"], without["got_extras"]):
        assert _eq(a, b)


# ---- 5. the run continues -------------------------------------------------------------------------------------------------------------------

def test_the_run_continues():
    """On the real remesher's mesh pair (the hand-adapted pair of cases.adapted_mesh has angles below regrid_angle by construction)."""
    r = _run("golden", True, False, False, True)
    (ang, flip, rg), crash = r["checks"]
    assert flip == 0 and rg == 0 and crash == 0 and r["checks"] == r["fresh_checks"]
    for k in r["after"]:
        assert _eq(r["after"][k], r["fresh_after"][k]), k
    assert np.abs(r["after"]["UM"]).max() > 0.


# ---- 6. a refused call leaves the handle alone ----------------------------------------------------------------------------------------------

def test_failure_leaves_the_handle_alone():
    xo, yo, to, xn, yn, tn, prev, ng = _pair("rect")
    p, lm, f = _fields(_global_mesh(xo, yo, to, ng), True)
    _, lm2, f2 = _fields(_global_mesh(xn, yn, tn, ng), True)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.step(); fe.synchronize()
    before = fe.get_state()
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    bad = [dict(old=np.zeros(lm.num_elements), transformation=7)]
    with pytest.raises(ValueError, match="unknown transformation"):                      # the wrapper ...
        fe.regrid(lm2, prev, ng, inputs, bad, moved=(xo, yo))
    with pytest.raises(dynamics.NxsError) as e:                                           # ... and the library behind it, before anything is launched
        fe.regrid(lm2, prev, ng, inputs, bad, moved=(xo, yo), validate=False)
    assert e.value.code == -1 and "transformation 7" in str(e.value)
    with pytest.raises(dynamics.NxsError) as e:
        fe.regrid(lm2, prev, ng, inputs, (), validate=False)
    assert e.value.code == -1 and "moved" in str(e.value)
    assert fe.lm is lm
    after = fe.get_state()
    for k in before:
        assert _eq(after[k], before[k]), k
    fe.step(); fe.synchronize()
    assert fe.checkFieldsFast() == 0 and not _eq(fe.get_state()["UM"], before["UM"])
    fe.close()


# ---- 7. a partitioned handle says why it cannot -----------------------------------------------------------------------------------------------

def test_multi_rank_is_refused():
    gm, p, g, lms, fields = cases.make_case("small", nparts=2)
    lm = lms[0]
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(fields[0])
    with pytest.raises(dynamics.NxsError) as e:
        fe.regrid(lm, None, 0, {k: fields[0][k] for k in dynamics.REGRID_INPUTS}, moved=(lm.coord_x, lm.coord_y))
    assert e.value.code == -4 and "halo lists" in str(e.value) and "rank 0 of 2" in str(e.value)
    assert fe.lm is lm and _eq(fe.get_state()["conc"], fields[0]["conc"])
    fe.close()
