"""The coupler's receive of nodal fields on the device (nxs_nodemap_*, nxs_dyn_nodes_coupled_*): 1. the weights against tests/golden/nodal_receive.npz, which the
REAL bamg made, the refusal in the notch, export / import; 2. the gather against nxs_regrid_interp_nodes on the same context, fed with the device's own source
rows, and the source kernel against the restatement (tests/nodal_receive_ref.py), both at the launch edges of a 256-thread block; the east/north pair within
section 6l's derived bound; 3. on the handle: the ocean's rows, one step against a fresh handle given the restatement's rows, the wave stress, what goes with the
mesh, and a handle that never attaches.  Every bar is bit for bit, NaN by position, except the east/north pair."""
import functools

import numpy as np
import pytest

import cases
import nodal_forcing_ref as NF
import nodal_receive_ref as R
import test_gpu_grid_remap as TG

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257)
STATE_KEYS = ("VT", "UM", "UT", "conc", "thick", "snow_thick", "damage", "ridge_ratio", "sigma0", "sigma1", "sigma2")
COEF = dict(a=[2., 1., -0.5, 1.], b=[0., 0.25, 0., -3.], factor=[1.5, -2., 1., 0.], bias=[0., 0.5, -0., 7.])


def coef(n):
    return {k: np.array(v[:n]) for k, v in COEF.items()}


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(R.GOLD))


def regrid_of(src):
    from nextsim_amd import interp
    return interp.Regrid((src["tri"] + 1).astype(np.int32), src["x"], src["y"])


@functools.lru_cache(maxsize=None)
def mapped(name):
    """(source, regrid context, node map) of a fixture case, made once"""
    from nextsim_amd import interp
    src = R.source(name)
    rg = regrid_of(src)
    return src, rg, interp.NodeMap.weights(rg, gold()["px_" + name], gold()["py_" + name])


def refused(call, *texts, code=-1):
    from nextsim_amd import dynamics
    with pytest.raises(dynamics.NxsError) as e:
        call()
    assert e.value.code == code and all(t in str(e.value) for t in texts), (e.value.code, str(e.value))
    return True


def polar():
    from nextsim_amd import dynamics
    m = dynamics.mapx_polar_north(**NF.MPP["NpsNextsim"])
    return m


def forward(lat, lon):
    from nextsim_amd import dynamics
    x, y = dynamics.mapx_forward(polar(), np.array([lat]), np.array([lon]), device=-1)
    return float(x[0]), float(y[0])


# ---- 1. weights, export, import ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "strip"])
def test_the_exported_weights_and_vertices_are_the_real_librarys(name):
    src, _, nm = mapped(name)
    g = gold()
    W = g["W_" + name]
    e, info = nm.export(), nm.info()
    assert info["N"] == W.shape[0] and info["nods_src"] == src["x"].size == e["nods_src"]
    assert info["beyond_hull"] == int((R.D.locate(src["x"], src["y"], src["tri"], g["px_" + name], g["py_" + name])[0] < 0).sum()) > 0
    assert (e["v"] >= 0).all() and (e["v"] < src["x"].size).all()
    assert np.array_equal(R.dense(e["v"], e["a"], src["x"].size).view(np.uint64), W.view(np.uint64))
    vr, _ = R.weights_from_dense(W, src["tri"])
    more = (W != 0).sum(1) > 1      # (at a hull vertex two weights are 0 and the reference's triangle depends on its walk)
    assert np.array_equal(e["v"][more], vr[more])
    d = R.awkward_data(src)
    for k in range(2):
        assert R.equal(R.apply(e["v"], e["a"], d[:, k]), g["Y_" + name][:, k])


def test_a_target_in_the_notch_is_refused_and_no_map_is_made():
    from nextsim_amd import interp
    src, g = R.source("notch"), gold()
    rg = regrid_of(src)
    fill = g["fill_notch"]
    assert refused(lambda: interp.NodeMap.weights(rg, g["px_notch"], g["py_notch"]), f"{fill.size} targets are outside of the source mesh but inside its convex hull",
                   f"target {fill.min()} ")
    keep = np.setdiff1d(np.arange(g["px_notch"].size), fill)      # without them the same source maps
    nm = interp.NodeMap.weights(rg, g["px_notch"][keep].copy(), g["py_notch"][keep].copy())
    assert nm.info()["N"] == keep.size
    nm.close(); rg.close()


def test_a_source_without_completion_is_refused():
    """a source the completion does not cover (tests/test_nodal_receive_abi.py asserts on the host that it does not): the interpolation itself goes on with the
    nearest-boundary-edge stand-in and says so; a node map is refused with the context's own reason -- it must never hold stand-in weights"""
    from nextsim_amd import interp
    x, y, tri, why = R.unmappable_source()
    rg = interp.Regrid((tri + 1).astype(np.int32), x, y)
    px, py = np.array([x.min() - 1e4, x.mean()]), np.array([y.min() - 1e4, y.mean()])
    _, info = rg.interp_nodes(np.zeros(x.size), px, py, return_info=True)
    assert info["completion_refused"] and why in info["completion_refused"] and info["num_stand_in"] >= 1
    assert refused(lambda: interp.NodeMap.weights(rg, px, py), "nodemap_create: the source triangulation has no convex completion", why, "a map never holds stand-in weights")
    assert refused(lambda: interp.NodeMap.weights(rg, px[1:], py[1:]), "no convex completion", why, "stand-in")      # even where every target is inside a triangle
    rg.close()


def test_import_of_export_gives_the_same_rows():
    from nextsim_amd import interp
    src, _, nm = mapped("strip")
    e = nm.export()
    nm2 = interp.NodeMap.import_(e)
    e2 = nm2.export()
    assert np.array_equal(e["v"], e2["v"]) and np.array_equal(e["a"].view(np.uint64), e2["a"].view(np.uint64)) and nm2.info()["N"] == nm.info()["N"]
    f = R.fields_case(src["G"], 2)
    for m in (nm, nm2):
        m.set_source(src["G"], src["reduced"])
    assert R.equal(nm.receive_rows(f), nm2.receive_rows(f))
    bad = dict(e, v=e["v"].copy()); bad["v"][3, 1] = e["nods_src"]
    assert refused(lambda: interp.NodeMap.import_(bad), "v1[3]", "is not a source node")
    nm2.close()


# ---- 2. source and gather ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("get", [False, True])
@pytest.mark.parametrize("in_device", [False, True])
@pytest.mark.parametrize("n_var", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["full", "strip"])
def test_the_gather_is_nxs_regrid_interp_nodes_on_the_devices_own_source_rows(name, n_var, in_device, get):
    src, rg, nm = mapped(name)
    g, k = gold(), coef(n_var)
    pairs = [] if n_var < 2 else [(0, 1)] if n_var < 4 else [(0, 1), (3, 2)]
    rot = R.uniform_rotation()
    nm.set_source(src["G"], src["reduced"], rotation="uniform", cos_m_diff_angle=rot[0], sin_m_diff_angle=rot[1])
    f = R.fields_case(src["G"], n_var)
    f[n_var - 1, 3 * R.NV + 4] = np.nan      # a NaN source node two rows inside the wet set: in no triangle behind a hull edge (see nodal_receive_ref.awkward_data)
    kw = dict(a=k["a"], b=k["b"], pairs=pairs, factor=k["factor"], bias=k["bias"], get=get)
    if in_device:
        N = nm.info()["N"]
        dev, out = [TG.Dev((src["G"],), f[v]) for v in range(n_var)], [TG.Dev((N,), np.full(N, -777.)) for _ in range(n_var)]
        assert nm.receive_rows([d.p.value for d in dev], in_device=True, out_device=[d.p.value for d in out], **kw) is None
        rows = np.stack([d.get() for d in out])
        for d in dev + out:
            d.free()
    else:
        rows = nm.receive_rows(f, **kw)
    stage = nm.debug_source(n_var)
    assert R.equal(stage, R.loaded_data(f, src["reduced"], k["a"], k["b"], pairs, rot))
    # the same context, the same data: InterpFromMeshToMesh2dx with isdefault = 0
    want = rg.interp_nodes(np.ascontiguousarray(stage.T), g["px_" + name], g["py_" + name], isdefault=False).T
    if get:
        with np.errstate(invalid="ignore"):
            want = np.stack([k["factor"][v] * want[v] + k["bias"][v] for v in range(n_var)])
    assert R.equal(rows, want)
    e = nm.export()
    assert R.equal(rows, R.receive(f, src["reduced"], k["a"], k["b"], e["v"], e["a"], pairs, rot, None, k["factor"] if get else None, k["bias"] if get else None))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("R_", SIZES)
def test_the_launch_edges_of_both_kernels(R_, N):
    """maps of 1, 255, 256, 257 targets over sources of 1, 255, 256, 257 reduced points: below, at and above one block of 256 threads"""
    from nextsim_amd import interp
    c, k = R.synthetic_case(R_, N, 3), coef(3)
    nm = interp.NodeMap.import_(dict(v=c["v"], a=c["w"], nods_src=R_))
    nm.set_source(c["G"], c["reduced"], rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=c["theta"])
    rows = nm.receive_rows(c["fields"], a=k["a"], b=k["b"], pairs=[(0, 1)], factor=k["factor"], bias=k["bias"], get=True)
    rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"])
    assert R.equal(nm.debug_source(3), R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"], [(0, 1)], rot))
    assert R.equal(rows, R.receive(c["fields"], c["reduced"], k["a"], k["b"], c["v"], c["w"], [(0, 1)], rot, None, k["factor"], k["bias"]))
    nm.close()


@pytest.mark.parametrize("N", SIZES)
def test_the_weights_kernel_at_the_launch_edges(N):
    from nextsim_amd import interp
    src, rg, _ = mapped("strip")
    g = gold()
    sel = np.linspace(0, g["px_strip"].size - 1, N).astype(int)
    nm = interp.NodeMap.weights(rg, g["px_strip"][sel].copy(), g["py_strip"][sel].copy())
    e = nm.export()
    assert np.array_equal(R.dense(e["v"], e["a"], src["x"].size).view(np.uint64), g["W_strip"][sel].view(np.uint64))
    nm.close()


@pytest.mark.parametrize("name", ["full", "strip"])
def test_both_rotations_are_bit_for_bit(name):
    src, _, nm = mapped(name)
    k = coef(3)
    f = R.fields_case(src["G"], 3)
    e = nm.export()
    plain = R.loaded_data(f, src["reduced"], k["a"], k["b"])
    for kw, rot in ((dict(rotation="uniform", cos_m_diff_angle=R.uniform_rotation()[0], sin_m_diff_angle=R.uniform_rotation()[1]), R.uniform_rotation()),
                    (dict(rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=src["theta"]), R.cos_sin_theta(R.MAP_ROTATION, src["theta"]))):
        nm.set_source(src["G"], src["reduced"], **kw)
        rows = nm.receive_rows(f, a=k["a"], b=k["b"], pairs=[(0, 1)])
        stage = nm.debug_source(3)
        assert R.equal(stage, R.loaded_data(f, src["reduced"], k["a"], k["b"], [(0, 1)], rot))
        assert not R.equal(stage[:2], plain[:2]) and R.equal(stage[2], plain[2])      # the pair turned, the scalar did not
        assert R.equal(rows, R.receive(f, src["reduced"], k["a"], k["b"], e["v"], e["a"], [(0, 1)], rot))
    nm.set_source(src["G"], src["reduced"])
    nm.receive_rows(f, a=k["a"], b=k["b"], pairs=[(0, 1)])
    assert R.equal(nm.debug_source(3), plain)                                        # no rotation: a pair is two scalars


def test_the_east_north_pair_is_within_the_derived_bound_and_the_gather_after_it_exact():
    src, _, nm = mapped("strip")
    k = coef(2)
    f = R.fields_case(src["G"], 2)
    f = np.where(np.abs(f) > 1e19, f, 0.3 * f)
    nm.set_source(src["G"], src["reduced"], east_west=True, lat=src["lat"], lon=src["lon"], mapx=polar())
    rows = nm.receive_rows(f, a=k["a"], b=k["b"], pairs=[(0, 1)], factor=k["factor"], bias=k["bias"], get=True)
    stage = nm.debug_source(2)
    det = {}
    want = R.loaded_data(f, src["reduced"], k["a"], k["b"], [(0, 1)], None, dict(lat=src["lat"], lon=src["lon"], forward=forward), details=det)
    bound = NF.bound_east_north(det[0])      # section 6l's derived bound, unchanged
    assert (np.abs(stage - want) <= bound[None, :]).all() and (bound > 0).any()
    assert not np.array_equal(stage, R.loaded_data(f, src["reduced"], k["a"], k["b"]))
    e = nm.export()
    with np.errstate(invalid="ignore"):
        assert R.equal(rows, np.stack([k["factor"][j] * R.apply(e["v"], e["a"], stage[j]) + k["bias"][j] for j in range(2)]))
    # east/north, THEN the rotation
    rot = R.cos_sin_theta(R.MAP_ROTATION, src["theta"])
    nm.set_source(src["G"], src["reduced"], rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=src["theta"], east_west=True, lat=src["lat"], lon=src["lon"], mapx=polar())
    nm.receive_rows(f, a=k["a"], b=k["b"], pairs=[(0, 1)])
    assert R.equal(nm.debug_source(2), np.stack(R.rotated(stage[0], stage[1], *rot)))
    nm.set_source(src["G"], src["reduced"])


def test_refusals_of_the_map():
    from nextsim_amd import interp
    src, rg, _ = mapped("strip")
    g = gold()
    nm = interp.NodeMap.weights(rg, g["px_strip"][:10].copy(), g["py_strip"][:10].copy())
    f = R.fields_case(src["G"], 2)
    assert refused(lambda: nm.receive_rows(f), "before nxs_nodemap_set_source", code=-4)
    assert refused(lambda: nm.debug_source(1), "no nxs_nodemap_receive_rows", code=-4)
    assert refused(lambda: nm.set_source(src["G"], src["reduced"][:-1]), "the map's source has")
    assert refused(lambda: nm.set_source(src["G"]), "reduced is NULL")
    bad = src["reduced"].copy(); bad[5] = src["G"]
    assert refused(lambda: nm.set_source(src["G"], bad), "reduced[5]")
    assert refused(lambda: nm.set_source(src["G"], src["reduced"], rotation="grid_theta"), "needs theta")
    assert refused(lambda: nm.set_source(src["G"], src["reduced"], rotation=7), "rotation_mode = 7")
    assert refused(lambda: nm.set_source(src["G"], src["reduced"], east_west=True), "needs lat, lon and map")
    assert refused(lambda: nm.set_source(src["G"], src["reduced"], east_west=True, lat=src["lat"], lon=src["lon"], mapx=polar(), delta_t=2.), "delta_t")
    nm.set_source(src["G"], src["reduced"])
    assert refused(lambda: nm.receive_rows([f[0]] * 5), "n_var = 5")
    assert refused(lambda: nm.receive_rows(f, pairs=[(0, 0)]), "pairs[0] = 0")
    assert refused(lambda: nm.receive_rows(np.stack([f[0], f[1], f[0]]), pairs=[(0, 1), (2, 1)]), "named by two pairs")
    assert refused(lambda: nm.debug_source(1), "no nxs_nodemap_receive_rows", code=-4)
    nm.close()


# ---- 3. on the handle ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def toy():
    """(params, local mesh, fields) of the toy mesh, and a node map of its nodes over the strip source"""
    gm, p, g, lms, fields = cases.make_case("toy")
    return p, lms[0], fields[0]


def toy_map(name="strip"):
    from nextsim_amd import interp
    p, lm, f = toy()
    src = R.source(name)
    x, y = np.asarray(lm.coord_x, np.float64), np.asarray(lm.coord_y, np.float64)
    cx, cy = 0.5 * (src["x"].min() + src["x"].max()), 0.5 * (src["y"].min() + src["y"].max())
    px = cx + 1.1 * np.ptp(src["x"]) * (x - 0.5 * (x.min() + x.max())) / np.ptp(x)
    py = cy + 1.1 * np.ptp(src["y"]) * (y - 0.5 * (y.min() + y.max())) / np.ptp(y)
    rg = regrid_of(src)
    nm = interp.NodeMap.weights(rg, px, py)
    nm.set_source(src["G"], src["reduced"], rotation="grid_theta", map_rotation=R.MAP_ROTATION, theta=src["theta"])
    return src, rg, nm


def free_bytes():
    import ctypes as C
    L = TG._hip()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert L.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def stepped(route):
    from nextsim_amd import dynamics
    p, lm, f = toy()
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    keep = route(fe)
    fe.step(); fe.synchronize()
    out = fe.get_state()
    launches = fe.timing()["substep_launches"]
    fe.close()
    for d in keep if isinstance(keep, list) else []:
        d.free()
    return out, launches


def ocean_fields(src):
    f = R.fields_case(src["G"], 3)
    f[0:2] *= 0.2; f[2] *= 0.1      # currents of decimetres per second, a sea surface of centimetres
    return np.where(np.abs(R.fields_case(src["G"], 3)) > 1e19, 1e20, f)


@pytest.mark.parametrize("in_device", [False, True])
def test_the_oceans_receive_on_the_handle_is_the_restatement_and_the_step_does_not_notice(in_device):
    p, lm, f = toy()
    Nn = lm.num_nodes
    src, rg, nm = toy_map()
    e = nm.export()
    fields = ocean_fields(src)
    a, b = np.array([1., 1., 0.5]), np.array([0., 0., 0.01])
    rot = R.cos_sin_theta(R.MAP_ROTATION, src["theta"])
    raw = R.receive(fields, src["reduced"], a, b, e["v"], e["a"], [(0, 1)], rot)
    factor, bias = {"ocean": 0.9, "ssh": 1.}, {"ocean": 0., "ssh": 0.02}
    got_rows = {}

    def new(fe):
        fe.nodes_coupled_attach("ocean", nm, a=a, b=b, factor=[3., 3., 3.], bias=[9., 9., 9.])      # (the ocean's factor / bias are set_forcing_time_rows's)
        dev = [TG.Dev((src["G"],), fields[v]) for v in range(3)] if in_device else []
        if in_device:
            fe.nodes_coupled_receive("ocean", [d.p.value for d in dev], device=True)
        else:
            fe.nodes_coupled_receive("ocean", fields)
        got_rows["get"] = fe.nodes_coupled_get("ocean")
        got_rows["forcing_get"] = fe.forcing_get(0, ["ocean_u", "ocean_v", "ssh"])
        fe.set_forcing(dict(wind=f["wind"], ocean=np.zeros(2 * Nn), ssh=np.zeros(Nn), element_depth=f["element_depth"]))      # wind and depth by the old call
        fe.set_forcing_time_rows({g: dict(mode="step", factor=factor[g], bias=bias[g]) for g in ("ocean", "ssh")})
        return dev

    def old(fe):
        with np.errstate(invalid="ignore"):
            f0 = dict(wind=f["wind"], ocean=np.concatenate([raw[0], raw[1]]), ssh=raw[2], element_depth=f["element_depth"])
        fe.set_forcing_pair(f0, f0)
        fe.set_forcing(dict(wind=f["wind"], ocean=np.zeros(2 * Nn), ssh=np.zeros(Nn), element_depth=f["element_depth"]))
        fe.set_forcing_time_rows({g: dict(mode="step", factor=factor[g], bias=bias[g]) for g in ("ocean", "ssh")})

    got, ln = stepped(new)
    assert R.equal(got_rows["get"], raw)
    assert all(R.equal(got_rows["forcing_get"][k], raw[j]) for j, k in enumerate(("ocean_u", "ocean_v", "ssh")))
    assert np.isfinite(raw).all() and np.abs(raw[:2]).max() < 5.
    want, lo = stepped(old)
    for k in STATE_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert ln == lo
    nm.close(); rg.close()


def test_the_wave_receive_is_set_wave_stress_with_the_restatements_vector():
    from nextsim_amd import dynamics
    p, lm, f = toy()
    src, rg, nm = toy_map()
    e = nm.export()
    fields = 0.05 * ocean_fields(src)[:2]
    fields = np.where(np.abs(fields) > 1e18, 1e20, fields)
    a, b, factor, bias = np.array([1., 1.]), np.array([0., 0.]), np.array([1., 1.]), np.array([0., 0.])
    rot = R.cos_sin_theta(R.MAP_ROTATION, src["theta"])
    vec = R.receive(fields, src["reduced"], a, b, e["v"], e["a"], [(0, 1)], rot, None, factor, bias)
    seen = {}

    def new(fe):
        fe.set_forcing(f)
        fe.nodes_coupled_attach("wave", nm, a=a, b=b, factor=factor, bias=bias)
        assert refused(lambda: fe.nodes_coupled_get("wave"), "no wave stress was received", code=-4)
        fe.nodes_coupled_receive("wave", fields)
        seen["rows"] = fe.nodes_coupled_get("wave")

    def old(fe):
        fe.set_forcing(f)
        fe.set_wave_stress(np.concatenate([vec[0], vec[1]]))

    def none(fe):
        fe.set_forcing(f)

    got, ln = stepped(new)
    assert R.equal(seen["rows"], vec) and np.isfinite(vec).all()
    want, lo = stepped(old)
    plain, _ = stepped(none)
    for k in STATE_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert ln == lo and not np.array_equal(got["VT"], plain["VT"])      # the stress was there, through the same kernel builds
    nm.close(); rg.close()


def test_refusals_on_the_handle_and_what_goes_with_the_mesh():
    from nextsim_amd import dynamics, interp
    p, lm, f = toy()
    src, rg, nm = toy_map()
    fields = ocean_fields(src)
    fe = dynamics.FiniteElementDynamics(p)
    assert refused(lambda: fe.nodes_coupled_attach("ocean", nm), "before set_mesh", code=-4)
    assert refused(lambda: fe.nodes_coupled_receive("ocean", fields), "before set_mesh", code=-4)
    fe.set_mesh(lm)
    assert refused(lambda: fe.nodes_coupled_receive("ocean", fields), "no ocean_cpl_nodes is attached", code=-4)
    assert refused(lambda: fe.nodes_coupled_get("wave"), "no wave_cpl_nodes is attached", code=-4)
    small = interp.NodeMap.import_(dict(v=nm.export()["v"][:-1], a=nm.export()["a"][:-1], nods_src=src["x"].size))
    assert refused(lambda: fe.nodes_coupled_attach("ocean", small), f"{lm.num_nodes - 1} targets", f"{lm.num_nodes} nodes")
    bare = interp.NodeMap.import_(nm.export())
    fe.nodes_coupled_attach("wave", bare)
    assert refused(lambda: fe.nodes_coupled_receive("wave", fields[:2]), "before nxs_nodemap_set_source", code=-4)
    fe.nodes_coupled_attach("ocean", nm)
    assert refused(lambda: fe.nodes_coupled_receive("ocean", fields[:2]), "has 3 fields, 2 were given")
    assert refused(lambda: fe.nodes_coupled_receive("ocean", [fields[0], None, fields[2]]), "field 1 (I_Vocn) is NULL")
    assert refused(lambda: fe.nodes_coupled_get("ocean"), "never received", code=-4)
    fe.nodes_coupled_receive("ocean", fields)
    first = fe.nodes_coupled_get("ocean")
    fe.nodes_coupled_detach("ocean")
    assert refused(lambda: fe.nodes_coupled_receive("ocean", fields), "no ocean_cpl_nodes is attached", code=-4)
    fe.nodes_coupled_attach("ocean", nm)
    fe.set_mesh(lm)                                                   # set_mesh detaches: the weights were the old mesh's
    assert refused(lambda: fe.nodes_coupled_receive("ocean", fields), "no ocean_cpl_nodes is attached", code=-4)
    assert refused(lambda: fe.nodes_coupled_receive("wave", fields[:2]), "no wave_cpl_nodes is attached", code=-4)
    fe.nodes_coupled_attach("ocean", nm)
    fe.nodes_coupled_receive("ocean", fields)
    assert R.equal(fe.nodes_coupled_get("ocean"), first)
    fe.close(); small.close(); bare.close()
    # nxs_dyn_regrid: an identity regrid of the rectangle detaches too
    x, y, tri, ng = cases.rect_mesh(25, 1)
    from nextsim_amd import forcing as F, mesh as M
    on_b = np.zeros(x.size, bool); on_b[:ng] = True
    gm = M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=on_b,
                      neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="rect")
    p2, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    lm2 = M.localize(gm, 1)[0]
    f2 = F.localize_fields(F.global_fields(gm, p2, "arctic", C_fix, C_alea), lm2, gm.num_nodes)
    c = R.synthetic_case(40, lm2.num_nodes, 3)
    nm2 = interp.NodeMap.import_(dict(v=c["v"], a=c["w"], nods_src=40))
    nm2.set_source(c["G"], c["reduced"])
    fe = dynamics.FiniteElementDynamics(p2)
    fe.set_mesh(lm2); fe.put_state(f2)
    fe.nodes_coupled_attach("ocean", nm2)
    fe.nodes_coupled_receive("ocean", c["fields"])
    before = fe.nodes_coupled_get("ocean")
    fe.regrid(lm2, np.arange(1, lm2.num_nodes + 1, dtype=np.float64), ng, {k: f2[k] for k in dynamics.REGRID_INPUTS}, (), moved=(lm2.coord_x, lm2.coord_y))
    assert refused(lambda: fe.nodes_coupled_receive("ocean", c["fields"]), "no ocean_cpl_nodes is attached", code=-4)
    fe.nodes_coupled_attach("ocean", nm2)
    fe.nodes_coupled_receive("ocean", c["fields"])
    assert R.equal(fe.nodes_coupled_get("ocean"), before)
    fe.close(); nm2.close(); nm.close(); rg.close()


def test_a_handle_that_never_attaches_keeps_its_bits():
    """one step of the toy mesh: a plain handle against a handle with an attachment that never receives, bit for bit and launch for launch (the receive is not part
    of the step), the attachment itself costing no device memory, and both against the CPU oracle, the yardstick smoke() uses"""
    p, lm, f = toy()

    def plain(fe):
        fe.set_forcing(f)

    def attached(fe):
        src, rg, nm = toy_map()
        fe.set_forcing(f)
        fe.synchronize()
        before = free_bytes()
        fe.nodes_coupled_attach("ocean", nm)      # attached, never received: nothing is allocated, nothing launched
        fe.nodes_coupled_attach("wave", nm)
        assert free_bytes() == before
        return src, rg, nm

    a, la = stepped(plain)
    b, lb = stepped(attached)
    for k in STATE_KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert la == lb
    from oracle import pyoracle as O
    ref = O.OracleRank(lm, p, f)
    ref.step()
    for k in ("VT", "sigma0", "damage", "conc", "thick", "UM"):
        scale = max(np.abs(ref.arr[k]).max(), 1e-300)
        assert np.abs(a[k] - ref.arr[k]).max() / scale < 1e-9, k
