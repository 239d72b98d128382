"""Nesting and the slab ocean's diffusion on the device (nxs_dyn_nesting_*, nxs_dyn_diffuse): 1. nesting_ice / nesting_dynamics with the linear function are
tests/nesting_ref.py bit for bit, with M_sigma / M_damage in their arrays and in the sub-step loop's records, BBM and EVP, and a following step does not notice by
which route the state was nudged; 2. the exponential function within two ulp of its one transcendental; 3. diffuse is the restatement bit for bit, its table is
nxs_mesh_element_connectivity, its rows stay where they are; 4. call order, what goes with the mesh, partitioned handles, device memory, the step's launches."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import nesting_ref as R
from nextsim_amd import _abi, forcing as F, mesh as M

pytestmark = pytest.mark.gpu

MESHES = ("tiny", "toy", "small", "odd")
BLOCK = 256
STATE_EL = ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "sigma0", "sigma1", "sigma2", "damage", "ridge_ratio")


def _rect(n, odd):
    """cases.rect_mesh(n, 1) as a local mesh; odd: without its last triangle (the odd Ne of tests/test_gpu_thermo_forcing.py)"""
    x, y, tri, ng = cases.rect_mesh(n, 1)
    if odd:
        tri = tri[:-1]
        assert np.array_equal(np.unique(tri), np.arange(x.size))
    on_b = np.zeros(x.size, bool); on_b[:ng] = True
    gm = M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=on_b,
                      neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="rect")
    p = F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE)
    p, C_fix, C_alea = F.scale_params_to_mesh(p, gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    return p, lm, F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes)


@functools.lru_cache(maxsize=None)
def _mesh(kind):
    """(params, local mesh, its fields); "oddnodes": a rectangle with an odd number of NODES (the second half of M_VT is then not 16-byte aligned)"""
    if kind == "odd":
        return _rect(24, True)
    if kind == "oddnodes":
        return _rect(23, False)
    gm, p, g, lms, fields = cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE)
    return p, lms[0], fields[0]


def _params(p, **over):
    q = p.copy()
    for k, v in over.items():
        setattr(q, k, v)
    return q


def _handle(kind, state=None, **over):
    from nextsim_amd import dynamics
    p, lm, f = _mesh(kind)
    fe = dynamics.FiniteElementDynamics(_params(p, **over))
    fe.set_mesh(lm)
    fs = dict(f, **(state or {}))
    fe.put_state(fs); fe.set_forcing(fs)
    return fe, lm, fs


def _refused(call, *texts, code=-4):
    from nextsim_amd import dynamics
    with pytest.raises(dynamics.NxsError) as e:
        call()
    assert e.value.code == code and all(t in str(e.value) for t in texts), (e.value.code, str(e.value))
    return True


def _same(got, want, keys, what):
    for k in keys:
        same = R.same_bits(got[k], want[k])
        assert same.all(), (what, k, np.flatnonzero(~same)[:5], np.asarray(got[k])[~same][:3], np.asarray(want[k])[~same][:3])


def _configure(fe, times, **over):
    cfg = dict(R.CFG, **over)
    fe.nesting_configure(**cfg)
    fe.nesting_time(R.time_arg(times))
    return cfg


def test_the_meshes_cover_the_kernels_edges():
    sizes = {k: _mesh(k)[1].num_elements for k in MESHES}
    assert any(n % 2 for n in sizes.values()), sizes                      # the scalar tail of the 16-byte pairs
    assert any(n < BLOCK for n in sizes.values()), sizes                  # less than one block
    assert any(n > 2 * 2 * BLOCK and n % (2 * BLOCK) for n in sizes.values()), sizes      # more than two blocks of 2 elements per lane, a ragged last one
    assert _mesh("oddnodes")[1].num_nodes % 2 == 1 and all(_mesh(k)[1].num_nodes % 2 == 0 for k in MESHES)
    assert all(_mesh(k)[1].num_nodes != n for k, n in sizes.items())


# ---- 1. the linear nudge is the restatement, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("times", [R.TIMES, R.TIMES_B], ids=["A", "B"])
@pytest.mark.parametrize("kind", MESHES + ("oddnodes",))
def test_the_linear_nudge_is_the_restatement_bit_for_bit_state_freshly_put(kind, times):
    p, lm, f = _mesh(kind)
    Ne, Nn = lm.num_elements, lm.num_nodes
    st0 = R.state(Ne, Nn)
    fe, lm, fs = _handle(kind, st0)
    cfg = _configure(fe, times)
    s0, s1 = R.snapshots(Ne, Nn, times, cfg["nudge_scale"])
    fe.nesting_pair(s0, s1)
    for which, s in ((0, s0), (1, s1)):                                    # the snapshots went up as they are, NaN and signed zeros included
        _same(fe.nesting_get(which), s, s.keys(), which)
    fe.nesting_ice()
    want = R.nesting_ice({k: fs[k].copy() for k in STATE_EL + ("VT",)}, (s0, s1), times, cfg, True)
    got = fe.get_state()
    _same(got, want, want.keys(), "nesting_ice")
    _same(got, fs, [k for k in got if k not in want], "a row nestingIce does not name")
    fe.nesting_dynamics()
    want = R.nesting_dynamics(want, (s0, s1), times, cfg)
    got = fe.get_state()
    _same(got, want, want.keys(), "nesting_dynamics")
    _same(got, fs, [k for k in got if k not in want], "a row nestingDynamics does not name")
    assert all(np.isfinite(got[k]).all() for k in want)                    # NaN / Inf of a STEP dataset's snapshot 1 reached nothing
    assert not R.same_bits(got["VT"], fs["VT"]).all() and not R.same_bits(got["sigma2"], fs["sigma2"]).all()
    fe.close()


def test_the_classic_category_leaves_the_young_rows_alone_and_does_not_need_their_snapshots():
    from nextsim_amd import dynamics
    p, lm, f = _mesh("tiny")
    Ne, Nn = lm.num_elements, lm.num_nodes
    st0 = R.state(Ne, Nn)
    fe = dynamics.FiniteElementDynamics(_params(p, ice_cat_type=_abi.NXS_ICECAT_CLASSIC))
    fe.set_mesh(lm)
    fs = dict(f, **st0)
    fe.put_state(fs)
    cfg = _configure(fe, R.TIMES, nest_dynamic_vars=False)
    s0, s1 = R.snapshots(Ne, Nn, R.TIMES, cfg["nudge_scale"])
    keep = ("dist", "thick", "conc", "snow_thick")
    fe.nesting_pair({k: s0[k] for k in keep}, {k: s1[k] for k in keep})
    fe.nesting_ice()
    want = R.nesting_ice({k: fs[k].copy() for k in STATE_EL + ("VT",)}, (s0, s1), R.TIMES, cfg, False)
    got = fe.get_state()
    _same(got, want, want.keys(), "classic")
    assert _refused(fe.nesting_dynamics, "nest_dynamic_vars")
    fe.close()


def _sane_nest(fs, Ne, Nn, scale):
    """an outer model close to the state: what a step can digest"""
    rng = np.random.default_rng(11)
    s0 = dict(dist=rng.uniform(0., 1.5 * scale, Ne), dist_nodes=rng.uniform(0., 1.5 * scale, Nn), thick=fs["thick"] * 0.9, conc=fs["conc"] * 0.95, snow_thick=fs["snow_thick"] * 1.1,
              h_young=fs["h_young"] * 0.9, conc_young=fs["conc_young"] * 0.9, hs_young=fs["hs_young"] * 0.9, damage=0.05 + fs["damage"] * 0.5, ridge_ratio=0.01 + fs["ridge_ratio"] * 0.5)
    s1 = dict(s0, thick=fs["thick"] * 1.05, conc=fs["conc"] * 0.9, damage=0.1 + fs["damage"] * 0.6)
    return s0, s1


SANE_TIMES = {"distance_elements": (R.STEP, 0., 0., 1., 0.), "ice_elements": (R.LINEAR, 0.25, 0.75, 1., 0.), "dynamics_elements": (R.LINEAR, 0.625, 0.375, 1., 0.),
              "distance_nodes": (R.STEP, 0., 0., 1., 0.), "nodes": (R.LINEAR, 0.5, 0.5, 1., 0.)}


@pytest.mark.parametrize("dyn", ["bbm", "evp"])
@pytest.mark.parametrize("kind", ["tiny", "odd", "small"])
def test_the_nudge_where_the_step_left_the_state_and_the_next_step_does_not_notice(kind, dyn):
    """A and B take one step; A goes the host's way (get_state, the numpy loops, put_state), B nudges on the device with M_sigma / M_damage in the records the
    sub-step loop left behind; then both step again.  Bit for bit after the nudge and after the second step: no second copy of sigma, damage or M_VT was left stale."""
    over = dict(dynamics_type=_abi.DYNAMICS_TYPES[dyn])
    A, lm, fs = _handle(kind, **over)
    B, _, _ = _handle(kind, **over)
    Ne, Nn = lm.num_elements, lm.num_nodes
    for fe in (A, B):
        fe.step()
    assert int(B.debug_array("update_launch")[0]) == 1                     # the records are home: k_update worked on them
    st1 = A.get_state()
    cfg = _configure(B, SANE_TIMES)
    s0, s1 = _sane_nest(fs, Ne, Nn, cfg["nudge_scale"])
    for k, j in (("sigma1", "sigma0"), ("sigma2", "sigma1"), ("sigma3", "sigma2")):
        s0[k], s1[k] = st1[j] * 0.8, st1[j] * 1.1
    s0["VT1"], s0["VT2"] = st1["VT"][:Nn] * 0.9, st1["VT"][Nn:] * 0.9
    s1["VT1"], s1["VT2"] = st1["VT"][:Nn] * 1.2, st1["VT"][Nn:] * 1.2
    B.nesting_pair(s0, s1)
    B.nesting_ice(); B.nesting_dynamics()
    want = {k: v.copy() for k, v in st1.items()}
    R.nesting_ice(want, (s0, s1), SANE_TIMES, cfg, True)
    R.nesting_dynamics(want, (s0, s1), SANE_TIMES, cfg)
    A.put_state(dict(fs, **want))
    for fe in (A, B):
        fe.step()
    assert int(B.debug_array("update_launch")[0]) == 1                     # ... and the second step found them there: nothing was unpacked in between
    a2, b2 = A.get_state(), B.get_state()
    _same(b2, a2, a2.keys(), ("after the second step", dyn))
    assert np.abs(a2["VT"]).max() > 0 and np.isfinite(a2["sigma0"]).all()
    # the nudge itself, from the records: a third pair of handles would cost a step each; B's twin C repeats B's first half
    Cc, _, _ = _handle(kind, **over)
    Cc.step()
    _configure(Cc, SANE_TIMES)
    Cc.nesting_pair(s0, s1)
    Cc.nesting_ice(); Cc.nesting_dynamics()
    got = Cc.get_state()
    _same(got, want, STATE_EL + ("VT",), ("records home", dyn))
    _same(got, st1, [k for k in got if k not in STATE_EL + ("VT",)], "a row the loops do not name")
    assert not R.same_bits(got["sigma0"], st1["sigma0"]).all() and not R.same_bits(got["damage"], st1["damage"]).all()
    for fe in (A, B, Cc):
        fe.close()


# ---- 2. the exponential function ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MESHES)
def test_the_exponential_nudge_is_within_two_ulp_of_its_transcendental(kind):
    """the device's exp is not the C library's: at most 2 ulp per transcendental, so |got - want| <= 2 * 2^-52 * |fNudge*q*(target - x)| + ulp(want)"""
    p, lm, f = _mesh(kind)
    Ne, Nn = lm.num_elements, lm.num_nodes
    st0 = R.state(Ne, Nn)
    times = R.TIMES
    worst = 0.
    for zero_dist in (False, True):
        fe, lm, fs = _handle(kind, st0)
        cfg = _configure(fe, times, nudge_function="exponential")
        s0, s1 = R.snapshots(Ne, Nn, times, cfg["nudge_scale"], zero_dist=zero_dist)
        fe.nesting_pair(s0, s1)
        fe.nesting_ice(); fe.nesting_dynamics()
        got = fe.get_state()
        before = {k: fs[k].copy() for k in STATE_EL + ("VT",)}
        want = R.nesting_dynamics(R.nesting_ice({k: v.copy() for k, v in before.items()}, (s0, s1), times, cfg, True), (s0, s1), times, cfg)
        if zero_dist:                                                      # fNudge = exp(-0.) = 1: bit for bit
            _same(got, want, want.keys(), "dist = 0")
            fe.close()
            continue
        fN = {False: R.f_nudge("exponential", R.get(times["distance_elements"], s0["dist"], s1["dist"]), cfg["nudge_scale"]),
              True: R.f_nudge("exponential", R.get(times["distance_nodes"], s0["dist_nodes"], s1["dist_nodes"]), cfg["nudge_scale"])}
        q, qd = np.float64(cfg["time_step"]) / cfg["nudge_timescale"], np.float64(cfg["dtime_step"]) / cfg["nudge_timescale"]
        source = dict(zip(STATE_EL, ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "sigma1", "sigma2", "sigma3", "damage", "ridge_ratio")))
        for k in want:
            if k == "VT":
                target = np.concatenate([R.get(times["nodes"], s0[v], s1[v]) for v in ("VT1", "VT2")])
                incr = np.concatenate([fN[True], fN[True]]) * qd * (target - before[k])
            else:
                incr = fN[False] * q * (R.get(times[R.dataset_of(source[k])], s0[source[k]], s1[source[k]]) - before[k])      # fNudge*q*(target - x)
            bound = 2. * 2. ** -52 * np.abs(incr) + np.spacing(np.abs(want[k]))
            err = np.abs(got[k] - want[k])
            assert (err <= bound).all(), (kind, k, np.flatnonzero(err > bound)[:5], (err / bound).max())
            worst = max(worst, float((err / bound).max()))
        fe.close()
    print(f"exponential nudge on {kind}: the largest |got - want| / bound is {worst:.3f}")


# ---- 3. diffuse ---------------------------------------------------------------------------------------------------------------------------------
def _ec(lm):
    from nextsim_amd import dynamics
    return dynamics.mesh_element_connectivity(lm.indices, lm.num_nodes)


def _shuffled(kind, seed=5):
    """the mesh with its elements renumbered at random: neighbours far apart, the table not banded"""
    import dataclasses
    p, lm, f = _mesh(kind)
    perm = np.random.default_rng(seed).permutation(lm.num_elements)
    lm2 = dataclasses.replace(lm, indices=np.ascontiguousarray(lm.indices.reshape(-1, 3)[perm].ravel()), ghost_nodes=np.ascontiguousarray(lm.ghost_nodes.reshape(-1, 3)[perm].ravel()))
    f2 = {k: (np.ascontiguousarray(v[perm]) if v.shape == (lm.num_elements,) else v) for k, v in f.items()}
    return p, lm2, f2


def _ocean(Ne, seed=0):
    rng = np.random.default_rng(seed + Ne)
    sst, sss = rng.normal(size=Ne) - 1., 33. + rng.normal(size=Ne)
    sst[Ne // 2] = -0.
    sss[0] = -0.
    return sst, sss


DIFF = dict(diffusivity_sst=1200., diffusivity_sss=350., dx=1500.5, dtime_step=900.)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("kind", MESHES)
def test_diffuse_is_the_restatement_bit_for_bit(kind, shuffle):
    from nextsim_amd import dynamics
    p, lm, f = _shuffled(kind) if shuffle else _mesh(kind)
    Ne = lm.num_elements
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    ec = _ec(lm)
    sst, sss = _ocean(Ne)
    fe.flux_put(sst=sst, sss=sss)
    rows0 = fe.flux_device_rows()
    for on in (dict(), dict(diffusivity_sss=0.), dict(diffusivity_sst=-3.), dict(diffusivity_sst=0., diffusivity_sss=0.)):
        c = dict(DIFF, **on)
        fe.diffusion_configure(**c)
        fe.flux_put(sst=sst, sss=sss)
        fe.diffuse()
        got = fe.flux_get(("sst", "sss"))
        for name, v, k in (("sst", sst, c["diffusivity_sst"]), ("sss", sss, c["diffusivity_sss"])):
            want = R.diffuse(v, k, c["dx"], c["dtime_step"], ec)
            assert R.same_bits(got[name], want).all(), (kind, shuffle, on, name, np.flatnonzero(~R.same_bits(got[name], want))[:5])
            assert (k > 0.) == (not R.same_bits(got[name], v).all())
    fe.diffusion_configure(**DIFF)                                           # twice in a row: the second call starts from the first's result
    fe.flux_put(sst=sst, sss=sss)
    fe.diffuse(); fe.diffuse()
    got = fe.flux_get(("sst", "sss"))
    assert R.same_bits(got["sst"], R.diffuse(R.diffuse(sst, 1200., 1500.5, 900., ec), 1200., 1500.5, 900., ec)).all()
    assert fe.flux_device_rows() == rows0 and rows0["sst"] and rows0["sss"] and not rows0["tice0"]      # the rows are where they were
    table = fe.debug_array("diffuse_table").reshape(Ne, 3)
    assert np.array_equal(table, np.where(np.isnan(ec), 0., ec) - 1.)        # nxs_mesh_element_connectivity, entry for entry (0-based, -1 on the boundary)
    if shuffle and Ne > 256:
        assert np.abs(table - np.arange(Ne)[:, None])[table >= 0].mean() > Ne / 8
    fe.close()


def test_the_table_is_built_again_for_another_mesh():
    from nextsim_amd import dynamics
    p, lm, f = _mesh("toy")
    p2, lm2, f2 = _mesh("small")
    assert lm.num_elements != lm2.num_elements
    fe = dynamics.FiniteElementDynamics(p)
    fe.diffusion_configure(**DIFF)                                           # the configuration is the handle's: it survives set_mesh
    assert _refused(fe.diffuse, "before set_mesh")
    for q, m in ((p, lm), (p2, lm2)):
        fe.set_params(q); fe.set_mesh(m)
        assert _refused(fe.diffuse, "sst was never put")
        sst, sss = _ocean(m.num_elements, 1)
        fe.flux_put(sst=sst)
        assert _refused(fe.diffuse, "sss was never put")
        fe.flux_put(sss=sss)
        fe.diffuse()
        got = fe.flux_get(("sst", "sss"))
        ec = _ec(m)
        assert R.same_bits(got["sst"], R.diffuse(sst, 1200., 1500.5, 900., ec)).all() and R.same_bits(got["sss"], R.diffuse(sss, 350., 1500.5, 900., ec)).all(), m.num_elements
        assert np.array_equal(fe.debug_array("diffuse_table").reshape(-1, 3), np.where(np.isnan(ec), 0., ec) - 1.)
    fe.close()


def test_diffuse_then_step_is_the_host_route():
    """M_sst / M_sss are read by neither explicitSolve() nor update()'s element loop: diffuse right before step is the reference's order (FE.cpp:3938-3939)"""
    A, lm, fs = _handle("small")
    B, _, _ = _handle("small")
    sst, sss = _ocean(lm.num_elements, 2)
    ec = _ec(lm)
    for fe in (A, B):
        fe.flux_put(sst=sst, sss=sss)
    B.diffusion_configure(**DIFF)
    B.diffuse(); B.step()
    A.flux_put(sst=R.diffuse(sst, 1200., 1500.5, 900., ec), sss=R.diffuse(sss, 350., 1500.5, 900., ec))
    A.step()
    _same(B.get_state(), A.get_state(), STATE_EL + ("VT", "UM"), "state")
    _same(B.flux_get(("sst", "sss")), A.flux_get(("sst", "sss")), ("sst", "sss"), "ocean")
    A.close(); B.close()


# ---- 4. the contract ----------------------------------------------------------------------------------------------------------------------------
def test_call_order_and_what_is_missing():
    from nextsim_amd import dynamics
    p, lm, f = _mesh("tiny")
    Ne, Nn = lm.num_elements, lm.num_nodes
    fe = dynamics.FiniteElementDynamics(p)
    assert _refused(fe.nesting_ice, "before nxs_dyn_nesting_configure") and _refused(fe.diffuse, "before nxs_dyn_diffusion_configure")
    assert _refused(lambda: fe.nesting_configure(**dict(R.CFG, nudge_function=5)), "nudge_function", "use exponential or linear", code=-1)
    assert _refused(lambda: fe.nesting_configure(**dict(R.CFG, nudge_timescale=0.)), "nudge_timescale", code=-1)
    assert _refused(lambda: fe.nesting_configure(**dict(R.CFG, nudge_scale=float("inf"))), "nudge_scale", code=-1)
    for bad, name in ((dict(dx=0.), "dx"), (dict(dx=float("nan")), "dx"), (dict(diffusivity_sst=float("inf")), "diffusivity_sst"), (dict(diffusivity_sss=float("nan")), "diffusivity_sss"),
                      (dict(dtime_step=float("inf")), "dtime_step")):
        assert _refused(lambda: fe.diffusion_configure(**dict(DIFF, **bad)), name, code=-1)
    fe.nesting_configure(**R.CFG)
    assert _refused(fe.nesting_ice, "needs set_mesh and put_state")
    assert fe.L.nxs_dyn_nesting_pair(fe.h, C.byref(_abi.NestingRows()), None) == -4 and b"before set_mesh" in fe.L.nxs_dyn_last_error(fe.h)
    fe.set_mesh(lm)
    assert _refused(fe.nesting_ice, "needs set_mesh and put_state")
    fe.put_state(f)
    assert _refused(fe.nesting_ice, "before nxs_dyn_nesting_time")
    assert _refused(lambda: fe.nesting_time({"nodes": dict(mode=7)}), "unknown mode 7", "nodes", code=-1)
    fe.nesting_time(R.time_arg(R.TIMES))
    assert _refused(fe.nesting_ice, "snapshot 0 of row dist is missing")
    s0, s1 = R.snapshots(Ne, Nn, R.TIMES, R.CFG["nudge_scale"])
    fe.nesting_pair(dict(dist=s0["dist"], conc=s0["conc"]))
    assert _refused(fe.nesting_ice, "row conc is LINEAR", "snapshot 1")
    fe.nesting_pair({}, dict(conc=s1["conc"]))
    assert _refused(fe.nesting_ice, "row thick is missing")
    fe.nesting_pair({k: s0[k] for k in ("thick", "snow_thick")}, {k: s1[k] for k in ("thick", "snow_thick")})
    assert _refused(fe.nesting_ice, "row conc_young is missing")              # the handle's ice_cat_type is YOUNG_ICE
    fe.nesting_pair({k: s0[k] for k in R.ICE_ROWS}, {k: s1[k] for k in R.ICE_ROWS})
    fe.nesting_ice()
    assert _refused(fe.nesting_dynamics, "row sigma1 is missing")
    fe.nesting_pair({k: s0[k] for k in R.DYN_ROWS})                           # dynamics_elements is STEP: snapshot 0 is enough
    assert _refused(fe.nesting_dynamics, "row dist_nodes is missing")
    fe.nesting_pair({k: s0[k] for k in _abi.NEST_NODE_ROWS}, dict(dist_nodes=s1["dist_nodes"], VT1=s1["VT1"]))
    assert _refused(fe.nesting_dynamics, "row VT2 is LINEAR")
    fe.nesting_pair({}, dict(VT2=s1["VT2"]))
    fe.nesting_dynamics()
    fe.nesting_time(R.time_arg({k: v for k, v in R.TIMES.items() if k != "nodes"}))
    assert _refused(fe.nesting_dynamics, "row VT1", "dataset nodes is OFF")
    assert _refused(lambda: fe.nesting_get(1, ["damage"]), "row damage of snapshot 1 is missing") and _refused(lambda: fe.nesting_get(2, ["dist"]), code=-1)
    with pytest.raises(KeyError):
        fe.nesting_pair(dict(nothing=np.zeros(Ne)))
    with pytest.raises(ValueError):
        fe.nesting_pair(dict(VT1=np.zeros(Ne)))
    fe.close()


def test_the_snapshots_go_with_the_mesh_and_the_configuration_stays():
    from nextsim_amd import dynamics
    p, lm, f = _mesh("tiny")
    p2, lm2, f2 = _mesh("toy")
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    cfg = _configure(fe, R.TIMES)
    s0, s1 = R.snapshots(lm.num_elements, lm.num_nodes, R.TIMES, cfg["nudge_scale"])
    fe.nesting_pair(s0, s1)
    fe.nesting_ice()
    fe.set_params(p2); fe.set_mesh(lm2)
    st0 = R.state(lm2.num_elements, lm2.num_nodes)
    fs = dict(f2, **st0)
    fe.put_state(fs)
    assert _refused(fe.nesting_ice, "row dist is missing") and _refused(lambda: fe.nesting_get(0, ["dist"]), "is missing")
    s0, s1 = R.snapshots(lm2.num_elements, lm2.num_nodes, R.TIMES, cfg["nudge_scale"])
    fe.nesting_pair(s0, s1)
    fe.nesting_ice(); fe.nesting_dynamics()                                   # configured and timed before set_mesh
    want = R.nesting_dynamics(R.nesting_ice({k: fs[k].copy() for k in STATE_EL + ("VT",)}, (s0, s1), R.TIMES, cfg, True), (s0, s1), R.TIMES, cfg)
    _same(fe.get_state(), want, want.keys(), "on the second mesh")
    fe.close()
    # nxs_dyn_regrid: an identity regrid of the rectangle
    p, lm, f = _mesh("oddnodes")
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    cfg = _configure(fe, R.TIMES)
    s0, s1 = R.snapshots(lm.num_elements, lm.num_nodes, R.TIMES, cfg["nudge_scale"])
    fe.nesting_pair(s0, s1)
    fe.nesting_ice()
    prev = np.arange(1, lm.num_nodes + 1, dtype=np.float64)
    fe.regrid(lm, prev, 96, {k: f[k] for k in dynamics.REGRID_INPUTS}, (), moved=(lm.coord_x, lm.coord_y))
    assert _refused(fe.nesting_ice, "row dist is missing")
    fe.close()


def test_a_partitioned_handle_nests_its_ghosts_and_refuses_to_diffuse():
    from nextsim_amd import dynamics
    gm, p, g, lms, fields = cases.make_case("small", nparts=2, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE)
    lm, f = lms[1], fields[1]
    assert lm.nranks == 2 and lm.num_nodes > lm.local_ndof and lm.ghost_nodes.any()      # there are ghost nodes, and elements that hold them
    Ne, Nn = lm.num_elements, lm.num_nodes
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    fs = dict(f, **R.state(Ne, Nn))
    fe.put_state(fs)
    cfg = _configure(fe, R.TIMES_B)
    s0, s1 = R.snapshots(Ne, Nn, R.TIMES_B, cfg["nudge_scale"])
    fe.nesting_pair(s0, s1)
    fe.nesting_ice(); fe.nesting_dynamics()
    want = R.nesting_dynamics(R.nesting_ice({k: fs[k].copy() for k in STATE_EL + ("VT",)}, (s0, s1), R.TIMES_B, cfg, True), (s0, s1), R.TIMES_B, cfg)
    _same(fe.get_state(), want, want.keys(), "all M_num_elements and M_num_nodes, ghosts included")
    fe.diffusion_configure(**DIFF)
    fe.flux_put(sst=np.zeros(Ne), sss=np.zeros(Ne))
    assert _refused(fe.diffuse, "this handle has halo lists set (rank 1 of 2)", "the gather / scatter of a partitioned run is not done here")
    fe.close()


def test_a_handle_that_never_calls_them_is_the_library_without_them():
    """device memory after set_mesh / put_state / step, the step's launches and its result: the same with the two configurations made (they allocate and launch
    nothing) as without; the snapshots and the table cost what they hold and go back with the mesh"""
    from nextsim_amd import dynamics
    L = dynamics.load_library()
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        a, b = C.c_size_t(), C.c_size_t()
        assert L.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
        return a.value
    gm, p, g, lms, fields = cases.make_case("10km")
    lm, f = lms[0], fields[0]
    Ne, Nn = lm.num_elements, lm.num_nodes

    def run(configure):
        fe = dynamics.FiniteElementDynamics(p)
        if configure:
            fe.nesting_configure(**R.CFG); fe.nesting_time(R.time_arg(R.TIMES)); fe.diffusion_configure(**DIFF)
        fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
        fe.step(); fe.synchronize()
        return fe, free_bytes(), (fe.timing()["substep_launches"], tuple(fe.debug_array("update_launch")), fe.traffic_model()["substep_kernel_name"], fe.traffic_model()["prep_kernel_name"])
    warm, _, _ = run(False)
    warm.close()
    a, free_a, plan_a = run(False)
    st_a = a.get_state()
    a.close()
    b, free_b, plan_b = run(True)
    assert free_b == free_a and plan_b == plan_a, (free_a, free_b, plan_a, plan_b)
    _same(b.get_state(), st_a, st_a.keys(), "a step with the configurations made")
    s0, s1 = R.snapshots(Ne, Nn, R.TIMES, R.CFG["nudge_scale"])
    b.nesting_pair(s0, s1)
    b.flux_put(sst=np.zeros(Ne), sss=np.ones(Ne))
    mid = free_bytes()
    b.diffuse(); b.synchronize()
    low = free_bytes()
    slack = 2 << 20                                                          # (the allocator hands out 2 MiB chunks: a row may sit in one that was open already)
    assert free_b - mid >= 8 * (24 * Ne + 6 * Nn) - slack and low <= mid, (free_b, mid, low)      # both snapshots of twelve [Ne] and three [Nn] rows
    b.set_mesh(lm)
    assert free_bytes() >= low + 8 * (24 * Ne + 6 * Nn) - slack, (low, free_bytes())      # the snapshots went with the mesh
    b.close()
