"""thermo()'s ice columns on the device (nxs_dyn_column: k_column, FE.cpp:5306-5411) against tests/column_ref.py, the line-by-line restatement (whose parity with a
binary of the reference is NOT pinned: model/ cannot be compiled here).  Under the BASIC ice-ocean flux no library call but the correctly rounded sqrt is
in the scope, and everything is required BIT FOR BIT: the 22 rows, tice0/1/2, tsurf_young, h_young, hs_young, over three consecutive fluxes() -> column(dt)
rounds in which the temperatures of one call feed the next.  Each round starts from the restatement's designed flux rows, written through the device_rows
door of nxs_dyn_fluxes_get, so the column is compared on identical inputs and the fluxes' libm tolerance does not enter.  Under EXCHANGE the device's hypot
enters Qio: the exactly-calm elements and the four rows before Qio stay bit for bit, every other row is measured as |device - restatement| / max(1,
|restatement|), printed, and bounded by four times the figure recorded on the MI355X (the factor the fluxes use: it covers a second ROCm's hypot), capped at
1e-9; the branches are the restatement's on every element (tests/test_column_ref.py shows that no element sits on an edge)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import column_ref as R
import fluxes_ref as FR
from nextsim_amd import _abi

pytestmark = pytest.mark.gpu

DT = R.DT
CAP = 1e-9
TOL_ROWS = R.ICE_ROWS + R.YOUNG_ROWS + R.IN_PLACE
# Largest |device - restatement| / max(1, |restatement|) recorded on the MI355X under EXCHANGE (ROCm 7.2 device hypot against glibc's) per row, over the prints of
# test_exchange (both meshes, both thermo types, three rounds); b = 4 * the figure, capped at 1e-9.  Key: the row, or "state:<name>" for a row written in place.
RECORDED = {
    "Qio": 6.62e-16, "hi": 1.73e-18, "hs": 0.00e+00, "hi_old": 0.00e+00, "del_hi": 1.73e-18, "del_hs_mlt": 0.00e+00, "mlt_hi_top": 3.47e-18,
    "mlt_hi_bot": 7.59e-19, "del_hi_s2i": 0.00e+00, "Qio_young": 5.50e-16, "hi_young": 0.00e+00, "hs_young": 0.00e+00, "hi_young_old": 0.00e+00,
    "del_hi_young": 2.71e-19, "del_hs_young_mlt": 0.00e+00, "mlt_hi_top_young": 0.00e+00, "mlt_hi_bot_young": 2.71e-19, "del_hi_s2i_young": 0.00e+00,
    "state:tice0": 1.15e-16, "state:tice1": 1.19e-16, "state:tice2": 3.77e-15, "state:tsurf_young": 0.00e+00, "state:h_young": 0.00e+00,
    "state:hs_young": 0.00e+00,
}
FLUX_NAMES = R.FLUX_IN + tuple(k + "_young" for k in R.FLUX_IN)
OPTIONS = (dict(freezingpoint_type="unesco"), dict(ocean_type="nudged"), dict(snowfall_source="snowfall"), dict(snowfall_source="precip_tair"), dict(mld_source="row"),
           dict(flooding=0), dict(ocean_type="nudged", mld_source="row", freezingpoint_type="unesco"))


def _key(i, k):
    return k if i < len(R.ROWS) else "state:" + k


def _bound(key):
    assert key in RECORDED, f"{key}: no figure recorded on the MI355X"
    return min(CAP, 4. * RECORDED[key])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def _bits(a, b):
    return bool(_same(a, b).all())


@functools.lru_cache(maxsize=None)
def _hip():
    """the HIP runtime the library itself has loaded: hipMemcpy is the way through the device_rows door"""
    from nextsim_amd import dynamics
    dynamics.load_library()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            lib.hipMemcpy.restype = C.c_int
            return lib
    return None


@functools.lru_cache(maxsize=None)
def _case(kind, young):
    gm, p, g, lms, fields = cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)
    lm, f = lms[0], fields[0]
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, strata, calm = R.make_inputs(lm.coord_x, lm.coord_y, tri)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    return p, lm, f, tri, inp, finp, calm


def _forcing_rows(inp, cfg):
    return dict(precip=inp["precip"], snow=inp["snowfall" if cfg["snowfall_source"] == "snowfall" else "snowfr"], ocean_temp=inp["ocean_temp"], ocean_salt=inp["ocean_salt"],
                mld=inp["mld"])


def _handle(kind, young, cfg=None, case_state=False, column_rows=True, **state_over):
    """A handle on mesh `kind` whose state, velocity and ocean are the inputs of column_ref.make_inputs (case_state: the ice state, M_VT and M_ocean stay the
    case's -- the tests that go on to a dynamics step), the fluxes configured and fed (the atmosphere of fluxes_ref.make_inputs with the column's tair), the
    column configured (cfg: a dict of column_ref.default_config, None = not configured) and its rows given.  Returns the handle and a private copy of the inputs."""
    from nextsim_amd import dynamics
    p, lm, f, tri, inp, finp, calm = _case(kind, young)
    inp = R.copy(inp)
    if case_state:
        inp.update({k: np.ascontiguousarray(f[k], np.float64).copy() for k in ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "VT", "ocean")})
    inp.update({k: np.ascontiguousarray(v, np.float64) for k, v in state_over.items()})
    f = dict(f, **{k: inp[k].copy() for k in ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "VT", "ocean")})
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1))   # (the drags stay: a later step must not see that fluxes() ran)
    fe.flux_set_atmosphere(tair=inp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"])
    fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], tsurf_young=inp["tsurf_young"], sst=inp["sst"], sss=inp["sss"]))
    if cfg is not None:
        fe.column_configure(**cfg)
        if column_rows:
            fe.column_set_forcing(**_forcing_rows(inp, cfg))
            fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    return fe, p, lm, f, tri, inp, calm


def _fluxes_then_feed(fe, ref_inp, young):
    """fluxes(), then the restatement's designed flux rows go into the device's through the device_rows door; without that door the device's own rows go to the
    restatement.  Either way both sides run the column on the same bits."""
    fe.fluxes()
    names = FLUX_NAMES if young else R.FLUX_IN
    got, dev = fe.fluxes_get(names, want_device=True)
    hip = _hip()
    if hip is None:
        for k in names:
            ref_inp[k] = got[k]
        return
    fe.synchronize()
    for k in names:
        a = np.ascontiguousarray(ref_inp[k], np.float64)
        assert dev[k] and a.size == fe.lm.num_elements
        assert hip.hipMemcpy(dev[k], a.ctypes.data, a.nbytes, 1) == 0
    back = fe.fluxes_get(names)
    for k in names:
        assert _bits(back[k], ref_inp[k]), k


def _device_state(fe, young):
    st = dict(fe.flux_get(("tice0", "tsurf_young")), **fe.column_get())
    s = fe.get_state()
    st["h_young"], st["hs_young"] = s["h_young"], s["hs_young"]
    return st


def _round(fe, cfg, tri, young, ref_inp, what, calm=None, measure=None):
    """one fluxes() -> column(dt) round on the device and in the restatement (ref_inp is updated in place); measure: a dict that collects the worst figures
    (EXCHANGE), None: bit for bit"""
    _fluxes_then_feed(fe, ref_inp, young)
    fe.column(DT)
    got = fe.column_rows()
    rows, rec = R.column(ref_inp, cfg, tri, young, DT)
    st = _device_state(fe, young)
    for i, k in enumerate(R.ROWS + R.IN_PLACE):
        dev, ref = (got[k], rows[k]) if i < len(R.ROWS) else (st[k], ref_inp[k])
        if not young and (k in R.YOUNG_ROWS or (i >= len(R.ROWS) and k in ("tsurf_young", "h_young", "hs_young"))):
            assert _bits(dev, ref), (what, k)
            continue
        if cfg["thermo_type"] == "zero_layer" and i >= len(R.ROWS) and k in ("tice1", "tice2"):
            assert _bits(dev, ref), (what, k)
            continue
        if measure is None or k in R.HEAD_ROWS:
            bad = np.flatnonzero(~_same(dev, ref))
            assert bad.size == 0, (what, _key(i, k), bad.size, bad[:5], dev[bad[:3]], ref[bad[:3]])
            continue
        assert _bits(dev[calm], ref[calm]), (what, k, "the calm elements")
        assert np.array_equal(np.isfinite(dev), np.isfinite(ref)), (what, k)
        ok = np.isfinite(ref)
        worst = float(np.max(np.abs(dev[ok] - ref[ok]) / np.maximum(1., np.abs(ref[ok]))))
        measure[_key(i, k)] = max(measure.get(_key(i, k), 0.), worst)
    if measure is not None:     # what of the branches shows in the rows: gone or kept, flooded, melted from below
        for sfx in ("", "_young") if young else ("",):
            hi, s2i, bot = (("hi", "del_hi_s2i", "mlt_hi_bot") if not sfx else ("hi_young", "del_hi_s2i_young", "mlt_hi_bot_young"))
            assert np.array_equal(got[hi] == 0, rows[hi] == 0) and np.array_equal(got[s2i] != 0, rows[s2i] != 0) and np.array_equal(got[bot] < 0, rows[bot] < 0), (what, sfx)
    return got, rows, rec, st


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_three_rounds_bit_for_bit(kind, thermo, young):
    cfg = R.default_config(thermo_type=thermo)
    fe, p, lm, f, tri, inp, calm = _handle(kind, young, cfg)
    assert kind != "toy" or lm.num_elements % 256 != 0          # a ragged last block
    ref_inp = R.copy(inp)
    first = None
    for call in range(3):
        got, rows, rec, st = _round(fe, cfg, tri, young, ref_inp, f"{kind} {thermo} young={young} round {call}")
        if call == 0:
            first = {k: st[k].copy() for k in R.IN_PLACE}
            assert np.abs(got["del_hi"]).max() > 0 and np.count_nonzero(got["hi"]) > lm.num_elements // 2
            if not young:
                assert not any(got[k].any() for k in R.YOUNG_ROWS)
    assert not np.array_equal(st["tice0"], first["tice0"])      # (each round fed the next)
    if young:
        assert not np.array_equal(st["h_young"], first["h_young"])
    fe.close()


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("over", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_every_option_bit_for_bit(over, thermo):
    cfg = R.default_config(thermo_type=thermo, **over)
    fe, p, lm, f, tri, inp, calm = _handle("small", True, cfg)
    ref_inp = R.copy(inp)
    got, rows, rec, st = _round(fe, cfg, tri, True, ref_inp, f"{over} {thermo}")
    base, _ = R.column(R.copy(inp), R.default_config(thermo_type=thermo), tri, True, DT)
    assert any(not np.array_equal(base[k], rows[k], equal_nan=True) for k in R.ROWS)            # (the option is not a no-op on these inputs)
    fe.close()


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_exchange(kind, thermo):
    cfg = R.default_config(thermo_type=thermo, qio_type="exchange")
    fe, p, lm, f, tri, inp, calm = _handle(kind, True, cfg)
    ref_inp = R.copy(inp)
    measure = {}
    for call in range(3):
        before = {k: inp[k].copy() for k in R.IN_PLACE} if call == 0 else _device_state(fe, True)
        own = R.copy(ref_inp)
        got, rows, rec, st = _round(fe, cfg, tri, True, ref_inp, f"exchange {kind} {thermo} round {call}", calm=calm, measure=measure)
        # the branches: the restatement started from the DEVICE's temperatures and young ice of the round before takes the branches it took from its own
        _, rec_dev = R.column(dict(own, **{k: before[k].copy() for k in R.IN_PLACE}), cfg, tri, True, DT)
        for k in rec:
            assert np.array_equal(rec[k], rec_dev[k]), (kind, thermo, call, k, np.flatnonzero(rec[k] != rec_dev[k])[:5])
    print(f"RECORD exchange {kind} {thermo}: " + ", ".join(f'"{k}": {v:.2e}' for k, v in measure.items()))
    assert set(measure) == {_key(i, k) for i, k in enumerate(R.ROWS + R.IN_PLACE) if k not in R.HEAD_ROWS and not (thermo == "zero_layer" and k in ("tice1", "tice2"))}
    for k, v in measure.items():
        assert v <= _bound(k), (kind, thermo, k, v, _bound(k))
    fe.close()


def test_call_order_and_the_device_rows():
    from nextsim_amd import dynamics
    cfg = R.default_config()
    fe, p, lm, f, tri, inp, calm = _handle("small", True, None)

    def refused(call, code=-4):
        with pytest.raises(dynamics.NxsError) as e:
            call()
        return e.value.code == code

    col = lambda: fe.column(DT)
    fe.fluxes()
    assert refused(col)                                         # before column_configure
    assert refused(fe.column_rows)                              # before the first column()
    with pytest.raises(dynamics.NxsError) as e:
        fe.column_configure(ocean_type="coupled")
    assert e.value.code == -1 and "OASIS" in str(e.value)
    fe.column_configure(**cfg)
    assert refused(col)                                         # no forcing row, no tice1 / tice2
    fe.column_set_forcing(**_forcing_rows(inp, cfg))
    assert refused(col)                                         # WINTON without tice1 / tice2
    fe.column_put(tice1=inp["tice1"])
    assert refused(col)                                         # ... without tice2
    assert refused(lambda: fe.column_get(("tice2",)))
    fe.column_put(tice2=inp["tice2"])
    assert refused(lambda: fe.column(0), -1) and refused(lambda: fe.column(-900), -1)           # dt <= 0
    fe.column(DT)
    got, dev = fe.column_rows(want_device=True)
    assert all(dev[k] for k in R.ROWS) and len(set(dev.values())) == len(R.ROWS)
    hip = _hip()
    if hip is not None:                                         # the device_rows pointers give what the host copies give
        for k in ("Qio", "del_hi", "hs_young", "del_hi_s2i_young"):
            a = np.empty(lm.num_elements)
            assert hip.hipMemcpy(a.ctypes.data, dev[k], a.nbytes, 2) == 0 and _bits(a, got[k]), k
    # a row the configuration needs and that was never given: mld under mld_source = row, ocean_temp / ocean_salt under a nudged ocean
    fe.column_configure(**dict(cfg, ocean_type="nudged"))
    fe.column(DT)                                               # (all five rows were given above)
    fe.set_mesh(lm)
    fe.put_state(f); fe.set_forcing(f)
    assert refused(col)                                         # after set_mesh: no fluxes() on this mesh; the configuration survived
    assert refused(fe.column_rows)
    finp = _case("small", True)[5]
    fe.flux_set_atmosphere(tair=inp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"])
    fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], tsurf_young=inp["tsurf_young"], sst=inp["sst"], sss=inp["sss"]))
    fe.fluxes()
    assert refused(col)                                         # the forcing rows and tice1 / tice2 went with the mesh
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    rows = _forcing_rows(inp, cfg)
    fe.column_set_forcing(**{k: v for k, v in rows.items() if k != "ocean_salt"})
    assert refused(col)                                         # nudged without ocean_salt
    fe.column_configure(**cfg)                                  # constant ocean, precip * snowfr, constant mld: precip and snow are enough
    fe.column(DT)
    fe.column_configure(**dict(cfg, mld_source="row"))
    fe.column(DT)                                               # (mld was given)
    fe.close()
    # the classic category: the nine young rows are zero and the young state is left alone
    cfg0 = R.default_config(thermo_type="zero_layer")
    fe, p, lm, f, tri, inp, calm = _handle("small", False, cfg0, column_rows=False)
    fe.column_set_forcing(precip=inp["precip"], snow=inp["snowfr"])
    fe.fluxes()
    fe.column(DT)                                               # ZERO_LAYER needs no tice1 / tice2
    got = fe.column_rows()
    assert not any(got[k].any() for k in R.YOUNG_ROWS) and np.abs(got["del_hi"]).max() > 0
    s = fe.get_state()
    assert _bits(s["h_young"], inp["h_young"]) and _bits(s["hs_young"], inp["hs_young"])
    fe.close()


def test_a_handle_that_never_configures_the_column_is_unchanged():
    """the traffic model and one step, bit for bit, with and without a configured column"""
    cfg = R.default_config()
    a, *_ = _handle("small", True, None, case_state=True)
    b, *_ = _handle("small", True, cfg, case_state=True)
    for fe in (a, b):
        fe.step(); fe.synchronize()
    assert a.traffic_model() == b.traffic_model()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert _bits(sa[k], sb[k]), k
    assert np.abs(sa["VT"]).max() > 0
    a.close(); b.close()


def test_the_next_step_reads_the_young_ice_the_column_wrote():
    """after column(), the next step is bit for bit that of a second handle given the restated h_young / hs_young through put_state"""
    cfg = R.default_config()
    fe, p, lm, f, tri, inp, calm = _handle("small", True, cfg, case_state=True)
    ref_inp = R.copy(inp)
    _round(fe, cfg, tri, True, ref_inp, "before the step")
    assert not np.array_equal(ref_inp["h_young"], inp["h_young"])
    fe.step(); fe.synchronize()
    fe2, *_ = _handle("small", True, None, case_state=True, h_young=ref_inp["h_young"], hs_young=ref_inp["hs_young"])
    fe2.step(); fe2.synchronize()
    sa, sb = fe.get_state(), fe2.get_state()
    for k in sa:
        assert _bits(sa[k], sb[k]), k
    assert np.abs(sa["VT"]).max() > 0
    fe.close(); fe2.close()
