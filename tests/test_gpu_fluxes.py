"""thermo()'s atmospheric bulk fluxes on the device (include/nxs_dyn.h: nxs_dyn_fluxes) against tests/fluxes_ref.py, the line-faithful restatement of
OWBulkFluxes, IABulkFluxes and their helpers (FE.cpp:5214-5277), on the meshes `small` and `toy` (2368 triangles: no multiple of 256), with and without the
young-ice category.

Tolerances.  Rows no math-library call reaches (fluxes_ref.NO_LIBM: the short-wave rows and the albedos), the all-zero young rows of the classic category and
the products with a calm element's zero wind speed (fluxes_ref.CALM_ZERO) are compared BIT FOR BIT.  Every other row and the four drags go through exp, pow,
log, atan, cbrt or hypot, the device's against the host's: |device - restatement| <= b * max(1, |restatement|) per row, b = four times the largest such
figure recorded on the MI355X over every test of this file (the table RECORDED below and DESIGN 6e) and never above 1e-9.  Every test prints what it measures.  tests/test_fluxes_ref.py shows that dropping the smallest term of the formulas moves some row by more than 1e-7 in the
same measure."""
import functools

import numpy as np
import pytest

import cases
import fluxes_ref as R
import means_ref
from nextsim_amd import _abi

pytestmark = pytest.mark.gpu

CAP = 1e-9
# Largest |device - restatement| / max(1, |restatement|) recorded on the MI355X (ROCm 7.2 device libm against glibc) per row and drag, over the prints of every
# test of this file (both meshes, both categories, three calls, every option); b = 4 * the figure.  The long-wave rows carry sigma T^4 of a few hundred W/m^2:
# one unit in the last place of such a value is 5.7e-14.
RECORDED = {
    "Qow": 1.14e-13, "Qlw_ow": 1.08e-13, "Qlh_ow": 3.24e-15, "Qsh_ow": 6.48e-16, "evap": 1.08e-19, "tau_ow": 8.67e-19,
    "Qia": 7.22e-14, "Qlwi": 1.14e-13, "Qlhi": 5.05e-14, "Qshi": 2.18e-15, "subl": 4.34e-19, "dQiadT": 1.82e-15,
    "Qia_young": 1.35e-13, "Qlw_young": 1.14e-13, "Qlh_young": 1.22e-13, "Qsh_young": 2.25e-15, "subl_young": 3.25e-19, "dQiadT_young": 1.59e-15,
    "drag_ui": 1.39e-17, "drag_ti": 1.21e-17, "drag_ui_young": 1.39e-17, "drag_ti_young": 1.04e-17,
}
LIBM_ROWS = tuple(k for k in R.ROWS if k not in R.NO_LIBM) + R.DRAGS
assert set(RECORDED) == set(LIBM_ROWS)


def _bound(name):
    assert name in LIBM_ROWS
    b = 4. * RECORDED[name]
    assert b <= CAP
    return b


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _measure(dev, ref):
    assert np.array_equal(np.isfinite(dev), np.isfinite(ref))
    ok = np.isfinite(ref)
    return float(np.max(np.abs(dev[ok] - ref[ok]) / np.maximum(1., np.abs(ref[ok])))) if ok.any() else 0.


@functools.lru_cache(maxsize=None)
def _case(kind, young):
    gm, p, g, lms, fields = cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)
    lm, f = lms[0], fields[0]
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, calm = R.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    return p, lm, f, tri, inp, calm


def _atmosphere(inp, cfg):
    hum = {"dewpoint": "dair", "sphuma": "sphuma", "mixrat": "mixrat"}[cfg["humidity_source"]]
    return dict(tair=inp["tair"], mslp=inp["mslp"], Qsw_in=inp["Qsw_in"], humidity=inp[hum], longwave=inp["Qlw_in" if cfg["longwave_source"] == "Qlw_in" else "tcc"])


def _handle(kind, young, cfg=None, flux_state=True, case_state=False, **field_over):
    """A handle on mesh `kind` whose wind, concentrations, snow and drags are the inputs of fluxes_ref.make_inputs, the fluxes configured (cfg: a dict of
    fluxes_ref.default_config, None = not configured) and their rows given; case_state: the concentrations and the snow stay the case's (the tests that go on
    to a dynamics step).  Returns the handle, the case and a private copy of the inputs."""
    from nextsim_amd import dynamics
    p, lm, f, tri, inp, calm = _case(kind, young)
    inp = R.copy(inp)
    inp.update({k: np.ascontiguousarray(v, np.float64) for k, v in field_over.items()})
    if case_state:
        inp.update({k: f[k].copy() for k in ("conc", "snow_thick", "conc_young", "hs_young")})
    f = dict(f, wind=inp["wind"], conc=inp["conc"], snow_thick=inp["snow_thick"], conc_young=inp["conc_young"], hs_young=inp["hs_young"],
             drag_ui=inp["drag_ui"].copy(), drag_ui_young=inp["drag_ui_young"].copy())
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    if cfg is not None:
        fe.flux_configure(**cfg)
        fe.flux_set_atmosphere(**_atmosphere(inp, cfg))
    if flux_state:
        fe.flux_put(**{k: inp[k] for k in _abi.FLUX_STATE})
    return fe, p, lm, f, tri, inp, calm


def _device_drags(fe):
    d = fe.flux_get(("drag_ti", "drag_ti_young"))
    d["drag_ui"], d["drag_ui_young"] = fe.debug_array("drag_ui"), fe.debug_array("drag_ui_young")
    return d


def _compare(what, got, drags, rows, ref_inp, calm, young):
    """one call's 25 rows and four drags against the restatement's"""
    worst = {}
    for k in R.ROWS:
        if k in R.NO_LIBM or (not young and k.endswith("_young")):
            assert _bits(got[k], rows[k]), (what, k)
            continue
        if k in R.CALM_ZERO:
            assert _bits(got[k][calm], rows[k][calm]), (what, k, "calm elements")
        worst[k] = _measure(got[k], rows[k])
    for k in R.DRAGS:
        if young or not k.endswith("_young"):
            worst[k] = _measure(drags[k], ref_inp[k])
        else:
            assert _bits(drags[k], ref_inp[k]), (what, k)
    print(what + ": " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= _bound(k), (what, k, v, _bound(k))
    return worst


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_three_calls_against_three_restatement_calls(kind, young):
    cfg = R.default_config()
    fe, p, lm, f, tri, inp, calm = _handle(kind, young, cfg)
    assert kind != "toy" or lm.num_elements % 256 != 0
    ref_inp = R.copy(inp)
    for call in range(3):
        before = _device_drags(fe) if call else {k: inp[k] for k in R.DRAGS}
        fe.fluxes()
        got, dev = fe.fluxes_get(want_device=True)
        rows, rec = R.fluxes(ref_inp, cfg, tri, young, p.quad_drag_coef_air)
        drags = _device_drags(fe)
        _compare(f"{kind} young={young} call {call}", got, drags, rows, ref_inp, calm, young)
        assert all(dev[k] for k in R.ROWS) and len(set(dev.values())) == len(R.ROWS)
        # the branches: the restatement started from the DEVICE's drags of the call before takes the branches it took from its own
        _, rec_dev = R.fluxes(dict(R.copy(inp), **{k: before[k].copy() for k in R.DRAGS}), cfg, tri, young, p.quad_drag_coef_air)
        for k in rec:
            assert np.array_equal(rec[k], rec_dev[k]), (kind, young, call, k, np.flatnonzero(rec[k] != rec_dev[k])[:5])
        if call == 0:
            first = {k: drags[k].copy() for k in R.DRAGS}
            for k in ("stable", "Linv_high", "Linv_low", "pond_active", "hs_positive", "Tsurf_warm", "subl_clamped", "Qlh_ow_clamped"):
                assert 0 < np.count_nonzero(rec[k]) < lm.num_elements, k
    assert not np.array_equal(drags["drag_ui"], first["drag_ui"]) and not np.array_equal(drags["drag_ti"], first["drag_ti"])   # (each call fed the next)
    # the calm elements: every flux finite, the turbulent ones zero
    for k in R.ROWS:
        assert np.all(np.isfinite(got[k][calm])), k
    for k in R.CALM_ZERO:
        assert not got[k][calm].any(), k
    fe.close()


@pytest.mark.parametrize("over", [dict(alb_scheme=1), dict(alb_scheme=2), dict(alb_scheme=4), dict(humidity_source="sphuma"), dict(humidity_source="mixrat"),
                                  dict(longwave_source="tcc"), dict(force_neutral_atmosphere=1)], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_every_option_on_small(over):
    cfg = R.default_config(**over)
    fe, p, lm, f, tri, inp, calm = _handle("small", True, cfg)
    ref_inp = R.copy(inp)
    fe.fluxes()
    got = fe.fluxes_get()
    rows, rec = R.fluxes(ref_inp, cfg, tri, True, p.quad_drag_coef_air)
    drags = _device_drags(fe)
    if over.get("force_neutral_atmosphere"):
        for k in R.DRAGS:
            assert _bits(drags[k], inp[k]), k
    _compare(str(over), got, drags, rows, ref_inp, calm, True)
    base, _ = R.fluxes(R.copy(inp), R.default_config(), tri, True, p.quad_drag_coef_air)
    assert any(not np.array_equal(base[k], rows[k]) for k in R.ROWS)            # (the option is not a no-op on these inputs)
    fe.close()


def test_means_update_reads_the_device_tau_ow():
    """after fluxes(), taux / tauy / taumod need no means_set_tau_ow and equal tests/means_ref.py fed the restatement's tau_ow"""
    from nextsim_amd import dynamics
    HYPOT_RTOL = 4e-16          # tests/test_gpu_means.py: the device's hypot against the C library's
    cfg = R.default_config()
    fe, p, lm, f, tri, inp, calm = _handle("small", True, cfg, case_state=True)
    nodal = ("taux", "tauy", "taumod", "wind_x")
    fe.means_configure((), nodal)
    with pytest.raises(dynamics.NxsError) as e:
        fe.means_update(1.)
    assert e.value.code == -4                                   # nothing attached yet
    fe.step()
    fe.fluxes()
    fe.means_update(0.5)
    fe.synchronize()
    rows, _ = R.fluxes(R.copy(inp), cfg, tri, True, p.quad_drag_coef_air)
    nec, _ = dynamics.mesh_connectivity(lm.indices, lm.num_nodes)
    ref = means_ref.MeansRef(lm.num_nodes, lm.num_elements, lm.local_nelements, True, (), nodal, nec)
    ref.update(0.5, fe.get_state(), diag=fe.get_diag(), wind=f["wind"], tau_ow=rows["tau_ow"])
    _, nod, _, _ = fe.means_get()
    # means_ref's own bound for these variables (tests/test_gpu_means.py) plus tau_ow's: tau_ow enters the second term linearly
    b_tau = _bound("tau_ow") / np.min(np.abs(rows["tau_ow"]))
    for k, name in enumerate(nodal):
        ok = np.isfinite(ref.nod[:, k])
        assert np.array_equal(np.isnan(nod[:, k]), np.isnan(ref.nod[:, k])), name
        if name == "wind_x":
            assert _bits(nod[:, k], ref.nod[:, k])
            continue
        err = np.abs(nod[ok, k] - ref.nod[ok, k])
        print(name, float(np.max(err / np.maximum(ref.nod_terms[ok, k], 1e-300))))
        assert np.all(err <= (16 * 2.0 ** -53 + b_tau + HYPOT_RTOL) * ref.nod_terms[ok, k]), name
        assert np.nanmax(np.abs(nod[:, k])) > 0
    fe.close()


def test_a_dynamics_step_uses_the_updated_drag():
    """D_tau_a of the step after fluxes() is, bit for bit, that of a handle given the updated drag_ui rows through put_state"""
    cfg = R.default_config()
    fe, p, lm, f, tri, inp, calm = _handle("small", True, cfg, case_state=True)
    fe.fluxes()
    drags = _device_drags(fe)
    assert not np.array_equal(drags["drag_ui"], inp["drag_ui"])
    fe.step(); fe.synchronize()
    a = fe.get_diag()["D_tau_a"]
    fe2, *_ = _handle("small", True, None, flux_state=False, case_state=True, drag_ui=drags["drag_ui"], drag_ui_young=drags["drag_ui_young"])
    fe2.step(); fe2.synchronize()
    b = fe2.get_diag()["D_tau_a"]
    fe3, *_ = _handle("small", True, None, flux_state=False, case_state=True)
    fe3.step(); fe3.synchronize()
    c = fe3.get_diag()["D_tau_a"]
    assert _bits(a, b) and not np.array_equal(a, c) and np.abs(a).max() > 0
    assert _bits(fe.get_state()["VT"], fe2.get_state()["VT"])
    for h in (fe, fe2, fe3):
        h.close()


def test_call_order():
    from nextsim_amd import dynamics
    cfg = R.default_config()
    fe, p, lm, f, tri, inp, calm = _handle("small", True, None)

    def refused():
        with pytest.raises(dynamics.NxsError) as e:
            fe.fluxes()
        return e.value.code == -4
    assert refused()                                            # before configure
    with pytest.raises(dynamics.NxsError) as e:
        fe.fluxes_get()
    assert e.value.code == -4
    with pytest.raises(dynamics.NxsError) as e:
        fe.flux_configure(alb_scheme=7)
    assert e.value.code == -1 and "alb_scheme" in str(e.value)
    fe.flux_configure(**cfg)
    assert refused()                                            # no atmosphere
    atm = _atmosphere(inp, cfg)
    fe.flux_set_atmosphere(**{k: v for k, v in atm.items() if k != "longwave"})
    assert refused()                                            # a missing atmosphere row
    fe.flux_set_atmosphere(longwave=atm["longwave"])
    fe.fluxes()                                                 # (the flux rows were put by _handle)
    fe.set_mesh(lm)
    fe.put_state(f); fe.set_forcing(f)
    assert refused()                                            # after set_mesh: every row is gone, the configuration is not
    fe.flux_set_atmosphere(**atm)
    fe.flux_put(**{k: inp[k] for k in _abi.FLUX_STATE if k != "sst"})
    assert refused()                                            # a missing flux row
    fe.flux_put(sst=inp["sst"])
    fe.fluxes()
    got = fe.fluxes_get(("Qow",))
    rows, _ = R.fluxes(R.copy(inp), cfg, tri, True, p.quad_drag_coef_air)
    assert _measure(got["Qow"], rows["Qow"]) <= _bound("Qow")
    back = fe.flux_get()
    for k in ("tice0", "tsurf_young", "sst", "sss", "pond_fraction", "lid_volume"):
        assert _bits(back[k], inp[k]), k
    fe.close()


def test_the_default_dynamics_path_is_untouched():
    """Two handles of THIS library: configured and run with force_neutral_atmosphere the fluxes leave the drags, so the step behind them gives the traffic
    model and the bits of a handle that never heard of them.  That the step of this library is the step of the one before it is what the existing suite shows
    (tests/test_gpu_parity.py against the oracle), not this test."""
    fe, p, lm, f, tri, inp, calm = _handle("small", True, R.default_config(force_neutral_atmosphere=1), case_state=True)
    fe.fluxes()
    fe.step(); fe.synchronize()
    fe2, *_ = _handle("small", True, None, flux_state=False, case_state=True)
    fe2.step(); fe2.synchronize()
    a, b = fe.get_state(), fe2.get_state()
    for k in a:
        assert _bits(a[k], b[k]), k
    ta, tb = fe.traffic_model(), fe2.traffic_model()
    assert ta == tb and ta["substep_unique_bytes"] > 0
    fe.close(); fe2.close()
