"""What goes with the mesh goes with it -- and nothing that vouches for freed device memory stays behind.

The handle keeps its per-mesh device memory in pools, each with one owner that lets go of the pool together with every pointer into it and every flag that
vouches for it; nxs_dyn_set_mesh, nxs_dyn_regrid and nxs_dyn_destroy call the owners.  These tests walk a live handle from one mesh to the next under every
sub-step family and with every optional buffer in place, and require (a) clean answers between the remesh and the next step -- the data-flow launch's error
word used to be read from the freed pair patches there -- and (b) afterwards the bits of a handle that only ever saw the second mesh.  "Equal" is bitwise, on
every key of get_state() and on the getters named.  Meshes: "small" (2.9 k triangles) and "toy" (2368), the smallest on which every patch kernel runs."""
import functools

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import fsd_ref as SR
from nextsim_amd import _abi, dynamics
from test_coupled_abi import smooth_wave_stress

pytestmark = pytest.mark.gpu

PAIR = {"fused": 2, "substeps_per_launch": 2, "pair_regs": 1}
# (options, the kernel of the sub-step loop on the first mesh)
FAMILIES = [({}, "k_substep_multi"), ({"fused": 0}, "k_sigma + k_solve_move"), ({"fused": 1}, "k_substep_fused"), ({"fused": 3}, "k_substep_multi"),
            (PAIR, "k_substep_pair"), (dict(PAIR, pair_flow=1), "k_substep_flow"), ({"fused": 4}, "k_substep_resident"), ({"smooth_depth": 5}, "k_substep_multi")]
INVALID, STATE = -1, -4     # NXS_ERR_INVALID, NXS_ERR_STATE


def _eq(a, b):
    """bitwise, NaN == NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def _assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert _eq(got[k], want[k]), f"{what}: {k}"


@functools.lru_cache(maxsize=None)
def _case(kind):
    gm, p, g, lms, fields = cases.make_case(kind)
    return p, lms[0], fields[0]


def _handle(p, options):
    fe = dynamics.FiniteElementDynamics(p)
    for k, v in options.items():
        fe.set_option(k, v)
    return fe


def _code(call):
    with pytest.raises(dynamics.NxsError) as e:
        call()
    return e.value.code


# ---- a. a remesh under every sub-step family -------------------------------------------------------------------------------------------------

def _two_steps(fe, f):
    fe.set_forcing(f); fe.step(); fe.step(); fe.synchronize()
    return fe.get_state(), fe.traffic_model()["substep_kernel_name"], fe.timing()["substep_launches"]


@functools.lru_cache(maxsize=None)
def _fresh(kind, options):
    p, lm, f = _case(kind)
    fe = _handle(p, dict(options))
    fe.set_mesh(lm); fe.put_state(f)
    out = _two_steps(fe, f)
    fe.close()
    return out


@pytest.mark.parametrize("second", ["toy", "small"])
@pytest.mark.parametrize("options,kernel", FAMILIES)
def test_remesh_under_every_family(options, kernel, second):
    p1, lm1, f1 = _case("small")
    p2, lm2, f2 = _case(second)
    fe = _handle(p1, options)
    fe.set_mesh(lm1); fe.put_state(f1)
    _, name, _ = _two_steps(fe, f1)
    assert name == kernel
    fe.set_params(p2)
    fe.set_mesh(lm2); fe.put_state(f2)
    got = fe.get_state()            # between the remesh and the next step: no launch can have given up, nothing of the old mesh is looked at
    for k in got:
        assert _eq(got[k], f2[k]), k
    after = _two_steps(fe, f2)
    fe.close()
    want = _fresh(second, tuple(sorted(options.items())))
    _assert_same(after[0], want[0], "state")
    assert after[1:] == want[1:]


def test_a_refused_pair_cut_is_tried_again_on_the_next_mesh():
    """pair_failed is a fact about ONE mesh.  With pair_nodes = 1024 no patch of "small" fits k_substep_pair (a workgroup solves at most 512 own nodes): the
    handle falls back to one sub-step per launch there.  All 56 nodes of "tiny" make one patch that fits: after set_mesh the cut is tried again, and the
    handle runs what a handle that only ever saw "tiny" runs."""
    options = dict(PAIR, pair_nodes=1024)
    p1, lm1, f1 = _case("small")
    p2, lm2, f2 = _case("tiny")
    fe = _handle(p1, options)
    fe.set_mesh(lm1); fe.put_state(f1)
    _, name, launches = _two_steps(fe, f1)
    assert name == "k_substep_fused" and launches == p1.substeps
    fe.set_params(p2)
    fe.set_mesh(lm2); fe.put_state(f2)
    after = _two_steps(fe, f2)
    fe.close()
    want = _fresh("tiny", tuple(sorted(options.items())))
    assert want[1] == "k_substep_pair" and want[2] == p2.substeps // 2
    _assert_same(after[0], want[0], "state")
    assert after[1:] == want[1:]


# ---- b. the whole handle at once -------------------------------------------------------------------------------------------------------------

NBINS = 3
MEANS = (["conc", "thick", "damage"], ["VT_x", "VT_y", "tauwix"])


def _everything(fe, kind):
    """Every optional buffer given on the handle's current mesh, one step, and every getter's answer."""
    p, lm, f = _case(kind)
    Ne, Nn = lm.num_elements, lm.num_nodes
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, _, _ = CR.make_inputs(lm.coord_x, lm.coord_y, tri)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    rng = np.random.default_rng(17)
    fe.put_state(f)
    f1 = dict(f, wind=1.5 * f["wind"], ocean=0.5 * f["ocean"], ssh=f["ssh"] + 0.01)
    fe.set_forcing_pair(f, f1); fe.set_forcing_time(0.25, 0.75)
    fe.set_wave_stress(smooth_wave_stress(lm))
    bins = SR.update_inputs(NBINS, Ne, True)
    fe.put_coupled(cum_damage=rng.uniform(0., 0.2, Ne), conc_fsd=bins["conc_fsd"])
    cfg = SR.default_config(NBINS, SR.standard_tables(NBINS), True)
    fe.fsd_configure(cfg["tables"], **SR.library_options(cfg))
    fe.fsd_put(conc_mech_fsd=bins["conc_mech_fsd"], cum_wave_damage=rng.uniform(0., 0.5, Ne))
    fe.flux_set_atmosphere(tair=inp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"])
    fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], tsurf_young=inp["tsurf_young"], sst=inp["sst"], sss=inp["sss"]))
    fe.fluxes()
    fe.column_set_forcing(precip=inp["precip"], snow=inp["snowfr"], ocean_temp=inp["ocean_temp"], ocean_salt=inp["ocean_salt"], mld=inp["mld"])
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    fe.column(CR.DT)
    cx, cy = lm.coord_x[tri].mean(1), lm.coord_y[tri].mean(1)
    fe.drifters_set(0, cx[:40], cy[:40], np.arange(40)); fe.drifters_set(1, cx[100:107], cy[100:107], np.arange(7) + 500)
    fe.set_option("trace_branches", 1)
    fe.step(); fe.means_update(1.0); fe.fsd_update(); fe.drifters_move(); fe.synchronize()
    el, nod, _, _ = fe.means_get()
    out = dict(fe.get_state(), means_el=el, means_nod=nod)
    out.update(fe.get_coupled(True, NBINS)); out.update(fe.fsd_get(NBINS, True))
    out.update({"flux:" + k: v for k, v in fe.fluxes_get().items()}); out.update({"col:" + k: v for k, v in fe.column_rows().items()})
    out.update(fe.flux_get()); out.update(fe.column_get())
    out.update({"trace:" + k: v for k, v in fe.branch_trace().items()})
    for s in (0, 1):
        out.update({f"drift{s}:{k}": v for k, v in fe.drifters_get(s).items()})
    return out


def _configured(p):
    """what is the handle's own and survives set_mesh: given once, before any mesh"""
    fe = dynamics.FiniteElementDynamics(p)
    fe.means_configure(*MEANS)
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1))
    fe.column_configure(**CR.default_config())
    return fe


def test_the_whole_handle_at_once():
    p1, lm1, _ = _case("small")
    p2, lm2, _ = _case("toy")
    fe = _configured(p1)
    fe.set_mesh(lm1)
    _everything(fe, "small")
    fe.set_params(p2)
    fe.set_mesh(lm2)
    # everything that goes with the mesh is gone, and says so
    assert _code(lambda: fe.get_coupled(True, NBINS)) == INVALID and _code(lambda: fe.get_coupled(False, NBINS)) == INVALID
    assert _code(lambda: fe.fsd_get(NBINS, False)) == INVALID and _code(lambda: fe.fsd_get(0, True)) == INVALID
    assert _code(fe.fluxes_get) == STATE and _code(fe.column_rows) == STATE
    assert _code(lambda: fe.flux_get(("tice0",))) == STATE and _code(fe.column_get) == STATE
    assert _code(lambda: fe.set_forcing_time(0.5, 0.5)) == STATE
    assert _code(fe.branch_trace) == STATE and _code(fe.get_state) == STATE and _code(fe.step) == STATE
    el, nod, _, _ = fe.means_get()
    assert el.shape == (lm2.num_elements, 3) and nod.shape == (lm2.num_nodes, 3) and not el.any() and not nod.any()
    assert fe.drifters_count(0) == 40 and fe.drifters_count(1) == 7       # the sets are the handle's
    got = _everything(fe, "toy")
    fresh = _configured(p2)
    fresh.set_mesh(lm2)
    want = _everything(fresh, "toy")
    _assert_same(got, want, "after the remesh")
    assert np.abs(got["UM"]).max() > 0. and got["trace:substeps"].max() == p2.substeps and got["means_el"].any() and got["flux:Qow"].any()
    fe.close(); fresh.close()


# ---- c. the same through nxs_dyn_regrid ------------------------------------------------------------------------------------------------------

def test_the_coupled_buffers_cross_a_regrid():
    import regrid_ref as RR
    import test_gpu_regrid_handle as T
    xo, yo, to, xn, yn, tn, prev, ng = T._pair("rect")
    p, lm, f = T._fields(T._global_mesh(xo, yo, to, ng), True)
    _, lm2, f2 = T._fields(T._global_mesh(xn, yn, tn, ng), True)
    Ne, Nn = lm.num_elements, lm.num_nodes
    rc = np.random.default_rng(12)      # (the coupled columns of test_gpu_regrid_handle._run)
    cum, fsd = rc.uniform(0., 0.2, Ne), np.ascontiguousarray(rc.dirichlet([1., 1., 1.], Ne).T * f["conc"])
    mech, cumw = np.ascontiguousarray(0.5 * fsd), rc.uniform(0., 0.5, Ne)
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, _, _ = CR.make_inputs(lm.coord_x, lm.coord_y, tri)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.put_coupled(cum_damage=cum, conc_fsd=fsd); fe.fsd_put(conc_mech_fsd=mech, cum_wave_damage=cumw)
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1)); fe.column_configure(**CR.default_config())
    fe.flux_set_atmosphere(tair=inp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"])
    fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], tsurf_young=inp["tsurf_young"], sst=inp["sst"], sss=inp["sss"]))
    fe.fluxes()
    fe.column_set_forcing(precip=inp["precip"], snow=inp["snowfr"], ocean_temp=inp["ocean_temp"], ocean_salt=inp["ocean_salt"], mld=inp["mld"])
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"]); fe.column(CR.DT)
    for _ in range(3):
        fe.step()
    fe.synchronize()
    st, cp, fs = fe.get_state(), fe.get_coupled(True, NBINS), fe.fsd_get(NBINS, True)
    xm, ym = lm.coord_x + st["UM"][:Nn], lm.coord_y + st["UM"][Nn:]
    # the host chain: cum_damage and the bins as the existing regrid test carries them; conc_mech_fsd and cum_wave_damage are two more plain columns
    # (NXS_TRANSFORM_NONE, bounded to [0, 1] / from below by 0) -- the chain's `none` extras do exactly that
    extras = [dict(old=fs["conc_mech_fsd"][b].copy(), transformation="none", min=0., max=1.) for b in range(NBINS)]
    extras.append(dict(old=fs["cum_wave_damage"].copy(), transformation="none", min=0.))
    ref, ref_extras, _ = RR.chain(st, (to, xm, ym), (tn, xn, yn), prev, ng, True, T._remap, T._interp, extras, cp, T.MU)
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    fe.regrid(lm2, prev, ng, inputs, (), moved=(xm, ym), freezingpoint_mu=T.MU)
    got = fe.get_state()
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
        assert _eq(got[k], ref[k]), k
    cp2, fs2 = fe.get_coupled(True, NBINS), fe.fsd_get(NBINS, True)
    assert _eq(cp2["cum_damage"], ref["cum_damage"]) and _eq(cp2["conc_fsd"], np.stack([ref[f"conc_fsd{b}"] for b in range(NBINS)]))
    assert _eq(fs2["conc_mech_fsd"], np.stack(ref_extras[:NBINS])) and _eq(fs2["cum_wave_damage"], ref_extras[NBINS])
    # the flux and column rows are the old mesh's: refused until they are given again
    assert _code(fe.fluxes_get) == STATE and _code(fe.column_rows) == STATE and _code(fe.fluxes) == STATE
    assert _code(lambda: fe.flux_get(("tice0",))) == STATE and _code(fe.column_get) == STATE
    # a step afterwards: a fresh handle given the regridded state and buffers
    fresh = dynamics.FiniteElementDynamics(p)
    fresh.set_mesh(lm2); fresh.put_state(dict(got, **inputs)); fresh.set_forcing(f2)
    fresh.put_coupled(cum_damage=cp2["cum_damage"], conc_fsd=cp2["conc_fsd"])
    fresh.fsd_put(conc_mech_fsd=fs2["conc_mech_fsd"], cum_wave_damage=fs2["cum_wave_damage"])
    fe.set_forcing(f2)
    for h in (fe, fresh):
        h.step(); h.synchronize()
    _assert_same(fe.get_state(), fresh.get_state(), "the step after the regrid")
    _assert_same(fe.get_coupled(True, NBINS), fresh.get_coupled(True, NBINS), "coupled")
    _assert_same(fe.fsd_get(NBINS, True), fresh.fsd_get(NBINS, True), "fsd")
    assert np.abs(fe.get_state()["UM"]).max() > 0.
    fe.close(); fresh.close()


# ---- d. the claims on the device's workgroup slots --------------------------------------------------------------------------------------------

def test_the_claim_goes_and_comes_with_the_mesh():
    """Two handles on one device, both asking for the resident loop.  The first holds the device's claim while it steps; set_mesh gives the claim back with the
    tables and the next step claims again; the second gets the loop once the first is closed (part (c) of test_resident_loop_survives_..., at the small size)."""
    p1, lm1, f1 = _case("small")
    p2, lm2, f2 = _case("toy")

    def launches(fe):
        fe.step(); fe.synchronize()
        return fe.timing()["substep_launches"]
    a, b = _handle(p1, {"fused": 4}), _handle(p1, {"fused": 4})
    a.set_mesh(lm1); a.put_state(f1); a.set_forcing(f1)
    b.set_mesh(lm1); b.put_state(f1); b.set_forcing(f1)
    assert launches(a) == 1
    a.set_params(p2)
    a.set_mesh(lm2); a.put_state(f2); a.set_forcing(f2)
    assert launches(a) == 1 and a.traffic_model()["substep_kernel_name"] == "k_substep_resident"
    a.close()                               # its claim goes with it
    assert launches(b) == 1 and b.traffic_model()["substep_kernel_name"] == "k_substep_resident"
    b.close()
