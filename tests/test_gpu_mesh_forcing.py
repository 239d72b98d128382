"""Forcing given on a triangulated source on the device (nxs_nodemap_load_rows, nxs_dyn_forcing_*_mesh, nxs_dyn_thermo_forcing_*_mesh): 1. load_rows against
tests/golden/mesh_forcing.npz, which the REAL bamg made, on every route and shape of the call; 2. the launch edges of a 256-thread block; 3. the gather against
nxs_regrid_interp_nodes on the same context, fed with the device's own staged rows; 4. both rotations bit for bit, the east/north pair within section 6l's derived
bound; 5. - 7. on the handle: the half-rows at the nodes and one step against a fresh handle given the same rows, the snapshot rows at the elements and the blend,
what goes with the mesh, a handle that never attaches; 8. every refusal.  Every bar is bit for bit, NaN by position, except the east/north pair."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import mesh_forcing_ref as MF
import nodal_forcing_ref as NF
import nodal_receive_ref as R
import test_gpu_grid_remap as TG
from test_gpu_nodal_receive import forward, free_bytes, polar, refused, regrid_of, toy

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(MF.GOLD))


@functools.lru_cache(maxsize=None)
def mapped(name, kind):
    """(source, regrid context, node map, targets) of a fixture case, made once"""
    from nextsim_amd import interp
    src = R.source(name)
    rg = regrid_of(src)
    px, py = MF.targets(src, kind)
    return src, rg, interp.NodeMap.weights(rg, px, py), (px, py)


def uniform(nm, src):
    rot = R.uniform_rotation()
    nm.set_source(src["G"], src["reduced"], rotation="uniform", cos_m_diff_angle=rot[0], sin_m_diff_angle=rot[1])
    return rot


def load(nm, G, f, n_step, co, pairs, route, skip=()):
    """load_rows by one of the four routes: fields on the host or the device, rows on the host or the device; the kept rows, in column order"""
    N, n_cols = nm.info()["N"], f.shape[0]
    kw = dict(n_step=n_step, pairs=pairs, **co)
    in_dev, out_dev = route in ("device", "in_only"), route in ("device", "out_only")
    dev = [TG.Dev((G,), f[c]) for c in range(n_cols)] if in_dev else []
    out = [None if c in skip else TG.Dev((N,), np.full(N, -777.)) for c in range(n_cols)] if out_dev else None
    got = nm.load_rows([d.p.value for d in dev] if in_dev else f, skip=skip, in_device=in_dev, out_device=[d.p.value if d else None for d in out] if out_dev else None, **kw)
    if out_dev:
        assert got is None
        rows = np.stack([d.get() for d in out if d])
    else:
        assert np.isnan(got[list(skip)]).all()      # a skipped column's host row is never written
        rows = got[[c for c in range(n_cols) if c not in skip]]
    for d in dev + [d for d in out or [] if d]:
        d.free()
    return rows


# ---- 1. load_rows against the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device", "in_only", "out_only"])
@pytest.mark.parametrize("kind", MF.KINDS)
@pytest.mark.parametrize("name", MF.SOURCES)
def test_load_rows_gives_the_real_librarys_bits(name, kind, route):
    src, _, nm, _ = mapped(name, kind)
    uniform(nm, src)
    f = MF.raw_fields(src["G"], src["reduced"])
    rows = load(nm, src["G"], f, 2, MF.coef(), MF.PAIRS, route)
    Y = gold()[f"Y_{kind}_{name}"]
    assert rows.shape == (6, Y.shape[0]) and R.equal(rows, Y.T)
    stage = nm.debug_load(6)
    assert R.equal(stage, MF.fixture_load(name)) and np.isfinite(stage).all()      # NaN zeroed, the land value never loaded


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("n_step", [1, 2])
@pytest.mark.parametrize("n_var", [1, 2, 3, 4])
def test_every_shape_of_the_load_and_a_skipped_column(n_var, n_step, route):
    src, _, nm, _ = mapped("strip", "nodes")
    rot = uniform(nm, src)
    c8 = MF.coef8()
    cols = [s * 4 + j for s in range(n_step) for j in range(n_var)]
    co = {k: c8[k][cols] for k in c8}
    f = MF.raw_fields(src["G"], src["reduced"], 8)[cols]
    pairs = [] if n_var < 2 else [(0, 1)] if n_var < 4 else [(0, 1), (3, 2)]
    n_cols = n_var * n_step
    skip = (n_cols - 1,) if n_cols > 1 else ()      # loaded (a pair needs it) but not gathered
    rows = load(nm, src["G"], f, n_step, co, pairs, route, skip)
    assert R.equal(nm.debug_load(n_cols), MF.loaded_data(f, src["reduced"], n_var, n_step, pairs=pairs, rotate=rot, **co))
    e = nm.export()
    want = MF.ingest(f, src["reduced"], n_var, n_step, e["v"], e["a"], pairs=pairs, rotate=rot, **co)
    assert R.equal(rows, want[[c for c in range(n_cols) if c not in skip]])
    if n_var == 3:      # the fixture's first snapshot when n_step == 1, both when 2 -- through the fourth-variable coefficient table's first three
        co3 = MF.coef(3, n_step)
        f3 = MF.raw_fields(src["G"], src["reduced"])[:3 * n_step]
        assert R.equal(load(nm, src["G"], f3, n_step, co3, MF.PAIRS, route), gold()["Y_nodes_strip"].T[:3 * n_step])


# ---- 2. launch edges ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("R_", SIZES)
def test_the_launch_edges_of_both_kernels(R_, N):
    """maps of 1, 255, 256, 257 targets over sources of 1, 255, 256, 257 reduced points: below, at and above one block of 256 threads"""
    from nextsim_amd import interp
    c, co = MF.synthetic_case(R_, N, 8), MF.coef8()
    nm = interp.NodeMap.import_(dict(v=c["v"], a=c["w"], nods_src=R_))
    nm.set_source(c["G"], c["reduced"], rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=c["theta"])
    pairs = [(0, 1), (3, 2)]
    rows = nm.load_rows(c["fields"], n_step=2, pairs=pairs, **co)
    rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"])
    assert R.equal(nm.debug_load(8), MF.loaded_data(c["fields"], c["reduced"], 4, 2, pairs=pairs, rotate=rot, **co))
    assert R.equal(rows, MF.ingest(c["fields"], c["reduced"], 4, 2, c["v"], c["w"], pairs=pairs, rotate=rot, **co))
    nm.close()


# ---- 3. the gather is k_interp's ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MF.KINDS)
@pytest.mark.parametrize("name", MF.SOURCES)
def test_the_gather_is_nxs_regrid_interp_nodes_on_the_devices_own_staged_rows(name, kind):
    src, rg, nm, (px, py) = mapped(name, kind)
    uniform(nm, src)
    f = MF.raw_fields(src["G"], src["reduced"], 8)
    rows = nm.load_rows(f, n_step=2, pairs=[(0, 1), (3, 2)], **MF.coef8())
    stage = nm.debug_load(8)
    want = rg.interp_nodes(np.ascontiguousarray(stage.T), px, py, isdefault=False).T      # the same context, the same data: InterpFromMeshToMesh2dx with isdefault = 0
    assert rows.shape == want.shape == (8, px.size) and R.equal(rows, want)


# ---- 4. the rotations and the east/north pair -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MF.SOURCES)
def test_both_rotations_are_bit_for_bit_in_both_forcing_steps(name):
    src, _, nm, _ = mapped(name, "elements")
    f, co = MF.raw_fields(src["G"], src["reduced"]), MF.coef()
    e = nm.export()
    plain = MF.loaded_data(f, src["reduced"], 3, 2, **co)
    for kw, rot in ((dict(rotation="uniform", cos_m_diff_angle=R.uniform_rotation()[0], sin_m_diff_angle=R.uniform_rotation()[1]), R.uniform_rotation()),
                    (dict(rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=src["theta"]), R.cos_sin_theta(R.MAP_ROTATION, src["theta"]))):
        nm.set_source(src["G"], src["reduced"], **kw)
        rows = nm.load_rows(f, n_step=2, pairs=MF.PAIRS, **co)
        stage = nm.debug_load(6)
        assert R.equal(stage, MF.loaded_data(f, src["reduced"], 3, 2, pairs=MF.PAIRS, rotate=rot, **co))
        for s in (0, 3):      # the pair turned in BOTH steps, the scalar in neither
            assert not R.equal(stage[s:s + 2], plain[s:s + 2]) and R.equal(stage[s + 2], plain[s + 2])
        assert R.equal(rows, MF.ingest(f, src["reduced"], 3, 2, e["v"], e["a"], pairs=MF.PAIRS, rotate=rot, **co))
    nm.set_source(src["G"], src["reduced"])
    nm.load_rows(f, n_step=2, pairs=MF.PAIRS, **co)
    assert R.equal(nm.debug_load(6), plain)      # no rotation: a pair is two scalars


def test_the_east_north_pair_is_within_the_derived_bound_and_the_gather_after_it_exact():
    src, _, nm, _ = mapped("strip", "nodes")
    f, co = MF.raw_fields(src["G"], src["reduced"]), MF.coef()
    f = np.where(np.abs(f) > 1e19, f, 0.3 * f)
    nm.set_source(src["G"], src["reduced"], east_west=True, lat=src["lat"], lon=src["lon"], mapx=polar())
    rows = nm.load_rows(f, n_step=2, pairs=MF.PAIRS, **co)
    stage = nm.debug_load(6)
    det = {}
    want = MF.loaded_data(f, src["reduced"], 3, 2, pairs=MF.PAIRS, east_west=dict(lat=src["lat"], lon=src["lon"], forward=forward), details=det, **co)
    for s in range(2):      # section 6l's derived bound, unchanged, in every forcing step
        bound = NF.bound_east_north(det[(s, 0)])
        assert (np.abs(stage[3 * s:3 * s + 2] - want[3 * s:3 * s + 2]) <= bound[None, :]).all() and (bound > 0).any()
        assert R.equal(stage[3 * s + 2], want[3 * s + 2])
    assert not np.array_equal(stage, MF.loaded_data(f, src["reduced"], 3, 2, **co))
    e = nm.export()
    assert R.equal(rows, np.stack([R.apply(e["v"], e["a"], stage[c]) for c in range(6)]))
    rot = R.cos_sin_theta(R.MAP_ROTATION, src["theta"])      # east/north, THEN the rotation
    nm.set_source(src["G"], src["reduced"], rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=src["theta"], east_west=True, lat=src["lat"], lon=src["lon"], mapx=polar())
    nm.load_rows(f, n_step=2, pairs=MF.PAIRS, **co)
    stage2 = nm.debug_load(6)
    for s in (0, 3):
        assert R.equal(stage2[s:s + 2], np.stack(R.rotated(stage[s], stage[s + 1], *rot)))
    nm.set_source(src["G"], src["reduced"])


# ---- 5. - 7. on the handle ---------------------------------------------------------------------------------------------------------------------------------------
def toy_map(kind, name="strip"):
    """a node map of the toy mesh's nodes or barycentres over a fixture source, the uniform rotation set"""
    from nextsim_amd import interp
    p, lm, f = toy()
    src = R.source(name)
    px, py = MF.scaled_to(src, np.asarray(lm.coord_x, np.float64), np.asarray(lm.coord_y, np.float64))
    if kind == "elements":
        t = np.asarray(lm.indices, np.int64).reshape(-1, 3) - 1
        px, py = (px[t[:, 0]] + px[t[:, 1]] + px[t[:, 2]]) / 3., (py[t[:, 0]] + py[t[:, 1]] + py[t[:, 2]]) / 3.
    rg = regrid_of(src)
    nm = interp.NodeMap.weights(rg, np.ascontiguousarray(px), np.ascontiguousarray(py))
    uniform(nm, src)
    return src, rg, nm


def ocean_fields(src):
    f = MF.raw_fields(src["G"], src["reduced"])
    return np.where(np.abs(f) > 1e19, f, 0.2 * f)      # currents of decimetres per second


def wind_grid(lm, seed=3):
    """a regular grid around the toy mesh with four columns (wind_u, wind_v of both snapshots): the older route, nxs_dyn_forcing_ingest"""
    rng = np.random.default_rng(seed)
    x, y = np.asarray(lm.coord_x), np.asarray(lm.coord_y)
    xs = np.linspace(x.min() - 0.02 * np.ptp(x), x.max() + 0.02 * np.ptp(x), 11)
    ys = np.linspace(y.min() - 0.02 * np.ptp(y), y.max() + 0.02 * np.ptp(y), 9)
    return xs, ys, 4. * rng.normal(size=(9, 11, 4))


def run_step(route):
    from nextsim_amd import dynamics
    p, lm, f = toy()
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    keep = route(fe)
    fe.step(); fe.synchronize()
    out, launches = fe.get_state(), fe.timing()["substep_launches"]
    fe.close()
    for d in keep if isinstance(keep, list) else []:
        d.free()
    return out, launches


TIME = {"wind": dict(mode="linear", fcoeff0=0.25, fcoeff1=0.75), "ocean": dict(mode="linear", fcoeff0=0.25, fcoeff1=0.75, factor=0.9),
        "ssh": dict(mode="linear", fcoeff0=0.25, fcoeff1=0.75, bias=0.02)}


@pytest.mark.parametrize("in_device", [False, True])
def test_the_ingest_at_the_nodes_fills_the_half_rows_and_the_step_does_not_notice(in_device):
    p, lm, f = toy()
    Nn = lm.num_nodes
    src, rg, nm = toy_map("nodes")
    e = nm.export()
    fields, co = ocean_fields(src), MF.coef()
    want = MF.ingest(fields, src["reduced"], 3, 2, e["v"], e["a"], pairs=MF.PAIRS, rotate=R.uniform_rotation(), **co)
    assert np.isfinite(want).all() and np.abs(want).max() < 5.
    xs, ys, wind = wind_grid(lm)
    seen = {}

    def new(fe):      # wind by the older route, ocean and ssh by this one: together they complete the pair
        fe.forcing_targets(0, lm.coord_x, lm.coord_y)
        fe.forcing_ingest(0, xs, ys, wind, ["wind_u", "wind_v", "wind_u", "wind_v"], [0, 0, 1, 1])
        assert refused(lambda: fe.set_forcing_time(0.5, 0.5), "before set_forcing_pair", code=-4)      # the pair is not complete yet
        fe.forcing_attach_mesh(1, nm)
        dev = [TG.Dev((src["G"],), fields[c]) for c in range(6)] if in_device else []
        fe.forcing_ingest_mesh(1, [d.p.value for d in dev] if in_device else fields, ["ocean_u", "ocean_v", "ssh"], pairs=MF.PAIRS, device=in_device, **co)
        seen[0], seen[1] = fe.forcing_get(0), fe.forcing_get(1)
        fe.set_forcing_time(0.5, 0.5)      # all ten half-rows are there: have_pair followed
        fe.set_forcing_time_rows(TIME)
        fe.set_element_depth(f["element_depth"])
        return dev

    def old(fe):
        snap = [dict(wind=np.concatenate([seen[s]["wind_u"], seen[s]["wind_v"]]), ocean=np.concatenate([want[3 * s], want[3 * s + 1]]), ssh=want[3 * s + 2],
                     element_depth=f["element_depth"]) for s in range(2)]
        fe.set_forcing_pair(snap[0], snap[1])
        fe.set_forcing_time(0.5, 0.5)
        fe.set_forcing_time_rows(TIME)
        fe.set_element_depth(f["element_depth"])

    got, ln = run_step(new)
    for s in range(2):
        assert all(R.equal(seen[s][k], want[3 * s + j]) for j, k in enumerate(("ocean_u", "ocean_v", "ssh"))), s
    assert not R.equal(seen[0]["ocean_u"], seen[1]["ocean_u"])
    ref, lo = run_step(old)
    assert set(got) == set(ref)
    for k in got:      # every key of the state
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert ln == lo
    nm.close(); rg.close()


def test_one_forcing_step_fills_snapshot_zero_only_for_a_step_dataset():
    from nextsim_amd import dynamics
    p, lm, f = toy()
    src, rg, nm = toy_map("nodes")
    e = nm.export()
    fields, co = ocean_fields(src)[:3], MF.coef(3, 1)
    want = MF.ingest(fields, src["reduced"], 3, 1, e["v"], e["a"], pairs=MF.PAIRS, rotate=R.uniform_rotation(), **co)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    fe.forcing_attach_mesh(0, nm)
    fe.forcing_ingest_mesh(0, fields, ["ocean_u", None, "ssh"], n_step=1, pairs=MF.PAIRS, **co)      # ocean_v skipped: the routes mix per half-row
    g0 = fe.forcing_get(0, ["ocean_u", "ssh"])
    assert R.equal(g0["ocean_u"], want[0]) and R.equal(g0["ssh"], want[2])
    assert refused(lambda: fe.forcing_get(0, ["ocean_v"]), "ocean_v of snapshot 0 is missing", code=-4)
    assert refused(lambda: fe.forcing_get(1, ["ssh"]), "ssh of snapshot 1 is missing", code=-4)
    assert refused(lambda: fe.set_forcing_time_rows({"ssh": dict(mode="linear")}), "ssh is LINEAR", code=-4)
    fe.set_forcing_time_rows({"ssh": dict(mode="step", factor=2., bias=0.5)})      # a `constant` / `nearest_daily` dataset: NXS_TF_STEP on snapshot 0
    assert refused(lambda: fe.set_forcing_time_rows({"ocean": dict(mode="step")}), "ocean is STEP", code=-4)
    fe.close(); nm.close(); rg.close()


def test_the_ingest_at_the_elements_fills_the_snapshot_rows_and_the_blend_does_not_notice():
    from nextsim_amd import dynamics
    p, lm, f = toy()
    src, rg, nm = toy_map("elements")
    assert nm.info()["N"] == lm.num_elements
    e = nm.export()
    fields, co = MF.raw_fields(src["G"], src["reduced"]), MF.coef()
    want = MF.ingest(fields, src["reduced"], 3, 2, e["v"], e["a"], **co)      # three scalars: sst, sss, mld
    names = ["ocean_temp", "ocean_salt", "mld"]
    time = {k: dict(mode="linear", fcoeff0=0.3, fcoeff1=0.7, factor=1. + 0.5 * j, bias=0.25 * j) for j, k in enumerate(names)}
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    fe.thermo_forcing_attach_mesh(2, nm)
    dev = [TG.Dev((src["G"],), fields[c]) for c in range(6)]
    fe.thermo_forcing_ingest_mesh(2, [d.p.value for d in dev], names, device=True, **co)
    for s in range(2):
        g = fe.thermo_forcing_get(s, names)
        assert all(R.equal(g[k], want[3 * s + j]) for j, k in enumerate(names)), s
    fe.thermo_forcing_time(time)
    got = fe.thermo_forcing_get(2, names)
    fe.thermo_forcing_ingest_mesh(2, fields, names, **co)      # host fields: the same rows
    assert all(R.equal(fe.thermo_forcing_get(1, names)[k], want[3 + j]) for j, k in enumerate(names))
    fe.close()
    fresh = dynamics.FiniteElementDynamics(p)
    fresh.set_mesh(lm); fresh.put_state(f)
    fresh.thermo_forcing_pair({k: want[j] for j, k in enumerate(names)}, {k: want[3 + j] for j, k in enumerate(names)})
    fresh.thermo_forcing_time(time)
    ref = fresh.thermo_forcing_get(2, names)
    assert all(R.equal(got[k], ref[k]) for k in names) and not R.equal(got["mld"], want[2])
    # n_step == 1: snapshot 0 only, NXS_TF_STEP
    fresh.set_mesh(lm)
    fresh.thermo_forcing_attach_mesh(0, nm)
    fresh.thermo_forcing_ingest_mesh(0, fields[:3], [None, "ocean_salt", "mld"], n_step=1, **MF.coef(3, 1))
    assert R.equal(fresh.thermo_forcing_get(0, ["mld"])["mld"], want[2])
    assert refused(lambda: fresh.thermo_forcing_get(1, ["mld"]), "mld of snapshot 1 is missing", code=-4)
    assert refused(lambda: fresh.thermo_forcing_get(0, ["ocean_temp"]), "ocean_temp of snapshot 0 is missing", code=-4)
    fresh.thermo_forcing_time({"mld": dict(mode="step")})
    fresh.close()
    for d in dev:
        d.free()
    nm.close(); rg.close()


def test_the_attachments_go_with_the_mesh():
    from nextsim_amd import dynamics, interp
    p, lm, f = toy()
    src, rg, nm = toy_map("nodes")
    _, rge, nme = toy_map("elements")
    fields, co = ocean_fields(src), MF.coef()
    node = lambda fe: fe.forcing_ingest_mesh(1, fields, ["ocean_u", "ocean_v", "ssh"], pairs=MF.PAIRS, **co)  # noqa: E731
    elem = lambda fe: fe.thermo_forcing_ingest_mesh(3, fields, ["ocean_temp", "ocean_salt", "mld"], **co)  # noqa: E731
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    fe.forcing_attach_mesh(1, nm); fe.thermo_forcing_attach_mesh(3, nme)
    node(fe); elem(fe)
    first, firste = fe.forcing_get(1, ["ocean_v"]), fe.thermo_forcing_get(1, ["mld"])
    fe.forcing_attach_mesh(1, None)      # NULL detaches; the rows that were ingested stay
    assert refused(lambda: node(fe), "set 1 has no node map on this mesh", code=-4) and R.equal(fe.forcing_get(1, ["ocean_v"])["ocean_v"], first["ocean_v"])
    fe.forcing_attach_mesh(1, nm)
    fe.set_mesh(lm)                      # set_mesh detaches both: the weights were the old mesh's
    assert refused(lambda: node(fe), "forcing_ingest_mesh: set 1 has no node map on this mesh", code=-4)
    assert refused(lambda: elem(fe), "thermo_forcing_ingest_mesh: set 3 has no node map on this mesh", code=-4)
    fe.forcing_attach_mesh(1, nm); fe.thermo_forcing_attach_mesh(3, nme)      # a map made on the new mesh attaches again
    node(fe); elem(fe)
    assert R.equal(fe.forcing_get(1, ["ocean_v"])["ocean_v"], first["ocean_v"]) and R.equal(fe.thermo_forcing_get(1, ["mld"])["mld"], firste["mld"])
    fe.close(); nm.close(); rg.close(); nme.close(); rge.close()
    # nxs_dyn_regrid: an identity regrid of the rectangle detaches too
    from nextsim_amd import forcing as F, mesh as M
    x, y, tri, ng = cases.rect_mesh(25, 1)
    on_b = np.zeros(x.size, bool); on_b[:ng] = True
    gm = M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=on_b,
                      neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="rect")
    p2, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    lm2 = M.localize(gm, 1)[0]
    f2 = F.localize_fields(F.global_fields(gm, p2, "arctic", C_fix, C_alea), lm2, gm.num_nodes)
    c, ce = MF.synthetic_case(40, lm2.num_nodes, 6), MF.synthetic_case(40, lm2.num_elements, 6)
    nm2, nm2e = interp.NodeMap.import_(dict(v=c["v"], a=c["w"], nods_src=40)), interp.NodeMap.import_(dict(v=ce["v"], a=ce["w"], nods_src=40))
    nm2.set_source(c["G"], c["reduced"]); nm2e.set_source(ce["G"], ce["reduced"])
    fe = dynamics.FiniteElementDynamics(p2)
    fe.set_mesh(lm2); fe.put_state(f2)
    fe.forcing_attach_mesh(0, nm2); fe.thermo_forcing_attach_mesh(0, nm2e)
    node2 = lambda: fe.forcing_ingest_mesh(0, c["fields"], ["ocean_u", "ocean_v", "ssh"], **co)  # noqa: E731
    elem2 = lambda: fe.thermo_forcing_ingest_mesh(0, ce["fields"], ["ocean_temp", "ocean_salt", "mld"], **co)  # noqa: E731
    node2(); elem2()
    before, beforee = fe.forcing_get(0, ["ssh"]), fe.thermo_forcing_get(0, ["ocean_salt"])
    fe.regrid(lm2, np.arange(1, lm2.num_nodes + 1, dtype=np.float64), ng, {k: f2[k] for k in dynamics.REGRID_INPUTS}, (), moved=(lm2.coord_x, lm2.coord_y))
    assert refused(node2, "set 0 has no node map on this mesh", code=-4) and refused(elem2, "set 0 has no node map on this mesh", code=-4)
    fe.forcing_attach_mesh(0, nm2); fe.thermo_forcing_attach_mesh(0, nm2e)
    node2(); elem2()
    assert R.equal(fe.forcing_get(0, ["ssh"])["ssh"], before["ssh"]) and R.equal(fe.thermo_forcing_get(0, ["ocean_salt"])["ocean_salt"], beforee["ocean_salt"])
    fe.close(); nm2.close(); nm2e.close()


def test_a_handle_that_never_attaches_keeps_its_bits():
    """one step of the toy mesh: a plain handle against a handle with attachments that never ingest, bit for bit and launch for launch (the ingest is not part of
    the step), the attachments costing no device memory; a map that never loads allocates no staging buffer; both steps against the CPU oracle"""
    p, lm, f = toy()

    def plain(fe):
        fe.set_forcing(f)

    def attached(fe):
        src, rg, nm = toy_map("nodes")
        _, rge, nme = toy_map("elements")
        fe.set_forcing(f)
        fe.synchronize()
        before = free_bytes()
        fe.forcing_attach_mesh(0, nm); fe.thermo_forcing_attach_mesh(0, nme)      # attached, never ingested: nothing is allocated, nothing launched
        assert free_bytes() == before
        assert refused(lambda: nm.debug_load(1), "no nxs_nodemap_load_rows", code=-4)
        attached.keep = (rg, nm, rge, nme)

    a, la = run_step(plain)
    b, lb = run_step(attached)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert la == lb
    from oracle import pyoracle as O
    ref = O.OracleRank(lm, p, f)
    ref.step()
    for k in ("VT", "sigma0", "damage", "conc", "thick", "UM"):
        scale = max(np.abs(ref.arr[k]).max(), 1e-300)
        assert np.abs(a[k] - ref.arr[k]).max() / scale < 1e-9, k


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_map():
    from nextsim_amd import _abi, interp
    src, rg, _, (px, py) = mapped("strip", "nodes")
    nm = interp.NodeMap.weights(rg, px[:10].copy(), py[:10].copy())
    f, co = MF.raw_fields(src["G"], src["reduced"]), MF.coef()
    assert refused(lambda: nm.load_rows(f, **co), "nodemap_load_rows: before nxs_nodemap_set_source", code=-4)
    assert refused(lambda: nm.debug_load(1), "no nxs_nodemap_load_rows", code=-4)
    nm.set_source(src["G"], src["reduced"])
    assert refused(lambda: nm.load_rows(np.stack([f[0]] * 5), n_step=1), "n_var = 5 (1 .. 4)")
    assert refused(lambda: nm.load_rows(f, pairs=[(0, 0)], **co), "pairs[0] = 0 is not another variable")
    assert refused(lambda: nm.load_rows(f, pairs=[(0, 3)], **co), "pairs[0] = 3 is not another variable (0 .. 2)")
    assert refused(lambda: nm.load_rows(f, pairs=[(0, 1), (2, 1)], **co), "named by two pairs")
    for key in ("scale_factor", "add_offset", "a", "b"):
        bad = {k: v.copy() for k, v in co.items()}
        bad[key][4] = np.inf if key != "b" else np.nan
        assert refused(lambda: nm.load_rows(f, **bad), "scale_factor, add_offset, a or b of column 4 is not finite")
    assert refused(lambda: nm.load_rows(f, skip=range(6), **co), "every column is skipped")
    dev = TG.Dev((src["G"],), f[0])
    assert refused(lambda: nm.load_rows([dev.p.value, None, dev.p.value], n_step=1, in_device=True), "field 1 (forcing step 0, variable 1) is NULL")
    dev.free()
    L, out = nm.L, (C.c_void_p * 8)()
    l, keep = nm._load_struct(f, 2, **co)
    row = np.empty(10)
    out[0] = row.ctypes.data
    last = lambda: L.nxs_interp_last_error().decode()  # noqa: E731
    assert L.nxs_nodemap_load_rows(nm.h, None, out, 0, None) == -1 and "NULL argument" in last()
    assert L.nxs_nodemap_load_rows(nm.h, C.byref(l), None, 0, None) == -1 and "NULL argument" in last()
    assert L.nxs_nodemap_load_rows(nm.h, C.byref(l), out, 8, None) == -1 and "flags = 0x8" in last()
    l.n_step = 3
    assert L.nxs_nodemap_load_rows(nm.h, C.byref(l), out, 0, None) == -1 and "n_step = 3 (1 or 2)" in last()
    l.n_step, l.n_var = 0, 3
    assert L.nxs_nodemap_load_rows(nm.h, C.byref(l), out, 0, None) == -1 and "n_step = 0" in last()
    l.n_step, l.n_var = 2, 0
    assert L.nxs_nodemap_load_rows(nm.h, C.byref(l), out, 0, None) == -1 and "n_var = 0" in last()
    l.n_var, l.fields = 3, None
    assert L.nxs_nodemap_load_rows(nm.h, C.byref(l), out, 0, None) == -1 and "NULL argument" in last()
    nm.load_rows(f, **co)
    assert refused(lambda: nm.debug_load(7), "n_cols = 7, the last load had 6") and nm.debug_load(2).shape == (2, src["reduced"].size)
    nm.set_source(src["G"], src["reduced"])      # a new source: the staged rows are not its
    assert refused(lambda: nm.debug_load(1), "no nxs_nodemap_load_rows", code=-4)
    del keep
    assert _abi.NXS_NODEMAP_MAX_LOAD == 8
    nm.close()


def test_refusals_on_the_handle():
    from nextsim_amd import dynamics, interp
    p, lm, f = toy()
    src, rg, nm = toy_map("nodes")
    _, rge, nme = toy_map("elements")
    fields, co = ocean_fields(src), MF.coef()
    rows, trows = ["ocean_u", "ocean_v", "ssh"], ["ocean_temp", "ocean_salt", "mld"]
    fe = dynamics.FiniteElementDynamics(p)
    assert refused(lambda: fe.forcing_attach_mesh(0, nm), "forcing_attach_mesh before set_mesh", code=-4)
    assert refused(lambda: fe.thermo_forcing_attach_mesh(0, nme), "thermo_forcing_attach_mesh before set_mesh", code=-4)
    assert refused(lambda: fe.forcing_ingest_mesh(0, fields, rows, **co), "forcing_ingest_mesh before set_mesh", code=-4)
    assert refused(lambda: fe.thermo_forcing_ingest_mesh(0, fields, trows, **co), "thermo_forcing_ingest_mesh before set_mesh", code=-4)
    fe.set_mesh(lm)
    assert refused(lambda: fe.forcing_ingest_mesh(0, fields, rows, **co), "set 0 has no node map on this mesh", code=-4)
    assert refused(lambda: fe.thermo_forcing_ingest_mesh(0, fields, trows, **co), "set 0 has no node map on this mesh", code=-4)
    assert refused(lambda: fe.forcing_attach_mesh(4, nm), "forcing_attach_mesh: set = 4 (0 .. 3)") and refused(lambda: fe.forcing_attach_mesh(-1, nm), "set = -1")
    assert refused(lambda: fe.thermo_forcing_attach_mesh(4, nme), "thermo_forcing_attach_mesh: set = 4 (0 .. 3)")
    assert refused(lambda: fe.forcing_ingest_mesh(4, fields, rows, **co), "forcing_ingest_mesh: set = 4")
    assert refused(lambda: fe.thermo_forcing_ingest_mesh(-1, fields, trows, **co), "thermo_forcing_ingest_mesh: set = -1")
    assert refused(lambda: fe.forcing_attach_mesh(0, nme), f"{lm.num_elements} targets", f"{lm.num_nodes} nodes (ghosts included)")      # the wrong target count
    assert refused(lambda: fe.thermo_forcing_attach_mesh(0, nm), f"{lm.num_nodes} targets", f"{lm.num_elements} elements (ghosts included)")
    bare = interp.NodeMap.import_(nm.export())
    fe.forcing_attach_mesh(2, bare)
    assert refused(lambda: fe.forcing_ingest_mesh(2, fields, rows, **co), "forcing_ingest_mesh:", "before nxs_nodemap_set_source", code=-4)
    fe.forcing_attach_mesh(0, nm); fe.thermo_forcing_attach_mesh(0, nme)
    assert refused(lambda: fe.forcing_ingest_mesh(0, fields, ["ocean_u", "ocean_v", 5], **co), "variable 2 goes to row 5 (-1 .. 4)")
    assert refused(lambda: fe.forcing_ingest_mesh(0, fields, ["ssh", "ocean_v", "ssh"], **co), "two variables go to row ssh")
    assert refused(lambda: fe.forcing_ingest_mesh(0, fields, [None, None, None], **co), "every variable is skipped")
    assert refused(lambda: fe.thermo_forcing_ingest_mesh(0, fields, ["mld", "ocean_salt", 10], **co), "variable 2 goes to row 10 (-1 .. 9)")
    assert refused(lambda: fe.thermo_forcing_ingest_mesh(0, fields, ["mld", "mld", None], **co), "two variables go to row mld")
    assert refused(lambda: fe.forcing_ingest_mesh(0, fields, rows, pairs=[(0, 0)], **co), "forcing_ingest_mesh:", "pairs[0] = 0")      # the map's refusals are passed on
    bad = dict(co, a=np.where(np.arange(6) == 1, np.nan, co["a"]))
    assert refused(lambda: fe.thermo_forcing_ingest_mesh(0, fields, trows, **bad), "thermo_forcing_ingest_mesh:", "column 1 is not finite")
    l, keep = nm._load_struct(fields, 2, **co)
    r = np.array([2, 3, 4], np.int32)
    ip = r.ctypes.data_as(C.POINTER(C.c_int32))
    for entry, h_map in ((fe.L.nxs_dyn_forcing_ingest_mesh, "forcing_ingest_mesh"), (fe.L.nxs_dyn_thermo_forcing_ingest_mesh, "thermo_forcing_ingest_mesh")):
        assert entry(fe.h, 0, C.byref(l), ip, 2) == -1 and f"{h_map}: flags = 0x2 (0 or NXS_REGRID_IN_DEVICE)" in (fe.L.nxs_dyn_last_error(fe.h) or b"").decode()      # NXS_REGRID_OUT_DEVICE is not the caller's
        assert entry(fe.h, 0, None, ip, 0) == -1 and entry(fe.h, 0, C.byref(l), None, 0) == -1 and entry(None, 0, C.byref(l), ip, 0) == -1
    l.n_step = 3
    assert fe.L.nxs_dyn_forcing_ingest_mesh(fe.h, 0, C.byref(l), ip, 0) == -1 and "n_step = 3" in (fe.L.nxs_dyn_last_error(fe.h) or b"").decode()
    del keep
    fe.forcing_ingest_mesh(0, fields, rows, pairs=MF.PAIRS, **co)      # ... and the handle still works
    fe.synchronize()
    fe.close(); bare.close(); nm.close(); rg.close(); nme.close(); rge.close()
