"""thermo()'s slab loop from new ice to tracers on the device (nxs_dyn_slab: k_slab, FE.cpp:5413-6133) against tests/slab_ref.py, the line-by-line restatement
(whose parity with a binary of the reference is NOT pinned: model/ cannot be compiled here).  Each round writes the restatement's designed flux rows AND column
rows through the device_rows doors of nxs_dyn_fluxes_get / nxs_dyn_column_get, so that neither earlier slice's tolerance enters, then calls slab(dt, clock).
Without the assimilation flux and newice_type 3 nothing in the scope calls more than sqrt and round, and everything is required BIT FOR BIT: the 29 rows, every
row written in place, time_relaxation_damage and the branch word, over three consecutive rounds whose state feeds the next.  Under use_assim_flux the device's
pow enters, under newice_type 3 its hypot: the branch word is the restatement's on every element (tests/test_slab_ref.py shows that no element sits on an
edge), every element that does not take the pow (has the exactly-calm nodes, or forms no new ice) is bit for bit, and the rest is measured as |device -
restatement| / max(1, |restatement|) per row, printed, and bounded by four times the figure recorded on the MI355X (the project's factor, from the fluxes and the
column: it covers a second ROCm's pow / hypot), capped at 1e-9; a recorded 0 means bits."""
import functools

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import slab_ref as R
from nextsim_amd import _abi

pytestmark = pytest.mark.gpu

DT = R.DT
CAP = 1e-9
ALB = FR.default_config()["ocean_albedo"]
ALL = dict.fromkeys(_abi.SLAB_CLOCK, 1)
# Largest |device - restatement| / max(1, |restatement|) recorded on the MI355X per row, over the prints of test_the_assimilation_flux (the device's pow against
# glibc's) and of test_newice_type_3 (its hypot), both meshes, both thermo types, three rounds; the bound is 4 * the figure, capped at 1e-9, and 0 means bits.
# Key: the row, or "state:<name>" for a row written in place.
RECORDED = {
    "assim": {
        "Qa": 0.00e+00, "Qsw": 0.00e+00, "Qlw": 0.00e+00, "Qsh": 0.00e+00, "Qlh": 0.00e+00, "Qo": 0.00e+00, "Qnosun": 0.00e+00, "Qsw_ocean": 0.00e+00,
        "Qassim": 6.71e-16, "delS": 0.00e+00, "fwflux_ice": 0.00e+00, "fwflux": 0.00e+00, "brine": 0.00e+00, "evap": 0.00e+00, "rain": 0.00e+00,
        "vice_melt": 0.00e+00, "del_vi_young": 0.00e+00, "del_hi": 0.00e+00, "del_hi_young": 0.00e+00, "newice": 0.00e+00, "mlt_top": 0.00e+00,
        "mlt_bot": 0.00e+00, "snow2ice": 0.00e+00, "albedo": 0.00e+00, "sialb": 0.00e+00, "del_ci_mlt_myi": 0.00e+00, "del_vi_mlt_myi": 0.00e+00,
        "del_ci_rplnt_myi": 0.00e+00, "del_vi_rplnt_myi": 0.00e+00, "state:conc": 0.00e+00, "state:thick": 0.00e+00, "state:snow_thick": 0.00e+00,
        "state:ridge_ratio": 0.00e+00, "state:conc_young": 0.00e+00, "state:h_young": 0.00e+00, "state:hs_young": 0.00e+00, "state:conc_myi": 0.00e+00,
        "state:thick_myi": 0.00e+00, "state:time_relaxation_damage": 0.00e+00, "state:sst": 1.52e-16, "state:sss": 0.00e+00, "state:pond_fraction": 0.00e+00,
        "state:lid_volume": 0.00e+00, "state:tice0": 0.00e+00, "state:tice1": 0.00e+00, "state:tice2": 0.00e+00, "state:pond_volume": 0.00e+00,
        "state:del_vi_tend": 0.00e+00, "state:freeze_days": 0.00e+00, "state:freeze_onset": 0.00e+00, "state:conc_summer": 0.00e+00,
        "state:thick_summer": 0.00e+00, "state:fyi_fraction": 0.00e+00, "state:age_det": 0.00e+00, "state:age": 0.00e+00,
    },
    "newice3": {
        "Qa": 2.18e-16, "Qsw": 0.00e+00, "Qlw": 0.00e+00, "Qsh": 0.00e+00, "Qlh": 0.00e+00, "Qo": 2.33e-16, "Qnosun": 0.00e+00, "Qsw_ocean": 0.00e+00,
        "Qassim": 0.00e+00, "delS": 0.00e+00, "fwflux_ice": 0.00e+00, "fwflux": 0.00e+00, "brine": 0.00e+00, "evap": 0.00e+00, "rain": 0.00e+00,
        "vice_melt": 0.00e+00, "del_vi_young": 0.00e+00, "del_hi": 0.00e+00, "del_hi_young": 0.00e+00, "newice": 0.00e+00, "mlt_top": 0.00e+00,
        "mlt_bot": 0.00e+00, "snow2ice": 0.00e+00, "albedo": 0.00e+00, "sialb": 0.00e+00, "del_ci_mlt_myi": 0.00e+00, "del_vi_mlt_myi": 0.00e+00,
        "del_ci_rplnt_myi": 0.00e+00, "del_vi_rplnt_myi": 0.00e+00, "state:conc": 2.78e-17, "state:thick": 4.34e-19, "state:snow_thick": 2.71e-19,
        "state:ridge_ratio": 0.00e+00, "state:conc_young": 0.00e+00, "state:h_young": 0.00e+00, "state:hs_young": 0.00e+00, "state:conc_myi": 0.00e+00,
        "state:thick_myi": 0.00e+00, "state:time_relaxation_damage": 0.00e+00, "state:sst": 1.16e-16, "state:sss": 0.00e+00, "state:pond_fraction": 0.00e+00,
        "state:lid_volume": 0.00e+00, "state:tice0": 0.00e+00, "state:tice1": 0.00e+00, "state:tice2": 0.00e+00, "state:pond_volume": 0.00e+00,
        "state:del_vi_tend": 0.00e+00, "state:freeze_days": 0.00e+00, "state:freeze_onset": 0.00e+00, "state:conc_summer": 0.00e+00,
        "state:thick_summer": 0.00e+00, "state:fyi_fraction": 2.78e-17, "state:age_det": 4.08e-16, "state:age": 0.00e+00,
    },
}


def _key(i, k):
    return k if i < len(R.ROWS) else "state:" + k


def _bound(table, key):
    assert key in RECORDED[table], f"{table} {key}: no figure recorded on the MI355X"
    return min(CAP, 4. * RECORDED[table][key])


@functools.lru_cache(maxsize=None)
def _case(kind, young):
    gm, p, g, lms, fields = cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)
    lm, f = lms[0], fields[0]
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, strata, calm = R.make_inputs(lm.coord_x, lm.coord_y, tri)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    return p, lm, f, tri, inp, finp, strata, calm


def _handle(kind, young, thermo="winton", opts=None, configure=True, sane=False, **kw):
    p, lm, f, tri, inp, finp, strata, calm = _case(kind, young)
    inp = R.sane_inputs(inp, f) if sane else R.copy(inp)
    ccfg = CR.default_config(thermo_type=thermo)
    cfg = R.category_config(young, **(opts or {}))
    fe, f = R.gpu_handle(p, lm, f, inp, finp, ccfg, cfg if configure else None, **kw)
    return fe, f, tri, inp, cfg, ccfg


def _round(fe, f, tri, ref, cfg, ccfg, young, flags, what, measure=None, exact=None):
    """one round on the device and in the restatement (ref is updated in place and then takes the device's rows: both start the next round from the same bits);
    measure: a dict that collects the worst figures, with `exact` the elements that must still be bit for bit; None: everything bit for bit"""
    clock = R.clock(**flags)
    got, st, words, before, after = R.gpu_round(fe, f, ref, DT, clock)
    rows, ref_words = R.slab(ref, cfg, ccfg, ALB, tri, young, DT, clock)
    assert np.array_equal(words, ref_words), (what, "branches", np.flatnonzero(words != ref_words)[:5], [hex(int(v)) for v in (words ^ ref_words)[words != ref_words][:5]])
    for k in _abi.FLUX_ROWS:                                    # the flux rows are read-only: fluxes_get answers the same after the call
        assert R.same_bits(before[k], after[k]).all(), (what, "flux row", k)
        assert k == "tau_ow" or R.same_bits(after[k], ref["F:" + k]).all(), (what, "flux row", k)
    for i, k in enumerate(R.ROWS + R.IN_PLACE):
        dev, want = (got[k], rows[k]) if i < len(R.ROWS) else (st[k], ref[k])
        same = R.same_bits(dev, want)
        if measure is None:
            bad = np.flatnonzero(~same)
            assert bad.size == 0, (what, _key(i, k), bad.size, bad[:5], dev[bad[:3]], want[bad[:3]])
            continue
        assert same[exact].all(), (what, _key(i, k), "the elements without the library call", np.flatnonzero(~same & exact)[:5])
        assert np.array_equal(np.isfinite(dev), np.isfinite(want)), (what, k)
        ok = np.isfinite(want)
        worst = float(np.max(np.abs(dev[ok] - want[ok]) / np.maximum(1., np.abs(want[ok]))))
        measure[_key(i, k)] = max(measure.get(_key(i, k), 0.), worst)
    for k in R.IN_PLACE:
        ref[k] = st[k].copy()
    return got, st, words


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_three_rounds_bit_for_bit(kind, thermo, young):
    fe, f, tri, inp, cfg, ccfg = _handle(kind, young, thermo)
    assert kind != "toy" or tri.shape[0] % 256 != 0             # a ragged last block
    ref = R.copy(inp)
    seen = np.uint32(0)
    for call, flags in enumerate(({}, dict(last_step_of_day=1), dict(first_step_of_day=1))):
        got, st, words = _round(fe, f, tri, ref, cfg, ccfg, young, flags, f"{kind} {thermo} young={young} round {call}")
        seen |= np.bitwise_or.reduce(words)
        if call == 0:
            first = {k: st[k].copy() for k in R.IN_PLACE}
            assert np.abs(got["vice_melt"]).max() > 0 and np.count_nonzero(st["conc"]) > tri.shape[0] // 2
    assert not np.array_equal(st["conc"], first["conc"]) and not np.array_equal(st["sst"], first["sst"]) and not np.array_equal(st["age"], first["age"])   # each round fed the next
    for k in ("supercooled", "melt", "limit", "ridge", "old_melt", "no_ice_tracers", "reset") + (("n4_sharp", "n4_no_room", "n4_not_filled") if young else ()):
        assert seen & np.uint32(R.BIT[k]), k
    fe.close()


OPTIONS = [(True, dict(melt_type=1), {}), (True, dict(temp_dep_healing=1, use_meltponds=1), {}), (True, dict(reset_by_date=1), ALL),
           (True, dict(reset_by_date=1, include_young_ice=0, equal_melting=0), dict(myi_reset_now=1)), (False, dict(newice_type=1), ALL), (False, dict(newice_type=2), {}),
           (False, dict(newice_type=2, melt_type=1, temp_dep_healing=1, use_meltponds=1), {})] + [(True, {}, {k: 1}) for k in _abi.SLAB_CLOCK]


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("young,opts,flags", OPTIONS, ids=lambda v: str(v))
def test_every_option_bit_for_bit(young, opts, flags, thermo):
    fe, f, tri, inp, cfg, ccfg = _handle("small", young, thermo, opts, put=R.SLAB_STATE)   # (conc_upd is not needed without the assimilation flux)
    ref = R.copy(inp)
    got, st, words = _round(fe, f, tri, ref, cfg, ccfg, young, flags, f"{opts} {flags} {thermo}")
    if opts.get("temp_dep_healing"):
        assert not np.array_equal(st["time_relaxation_damage"], inp["time_relaxation_damage"]) and (st["time_relaxation_damage"] == 1e36).any()
        assert R.took(words, "lid_exists").any() and R.took(words, "lid_forms").any() and R.took(words, "lid_removed").any() and R.took(words, "pond_flushed").any()
    else:
        assert np.array_equal(st["time_relaxation_damage"], inp["time_relaxation_damage"]) and np.array_equal(st["pond_volume"], inp["pond_volume"])
    fe.close()


def _measured(table, kind, thermo, young, opts, exact_of):
    fe, f, tri, inp, cfg, ccfg = _handle(kind, young, thermo, opts)
    ref = R.copy(inp)
    measure = {}
    for call in range(3):
        start = R.copy(ref)
        _, words0 = R.slab(R.copy(start), cfg, ccfg, ALB, tri, young, DT, R.clock())
        _round(fe, f, tri, ref, cfg, ccfg, young, {}, f"{table} {kind} {thermo} round {call}", measure=measure, exact=exact_of(start, words0))
    print(f"RECORD {table} {kind} {thermo}: " + ", ".join(f'"{k}": {v:.2e}' for k, v in measure.items()))
    assert set(measure) == {_key(i, k) for i, k in enumerate(R.ROWS + R.IN_PLACE)}
    fe.close()
    for k, v in measure.items():
        assert v <= _bound(table, k), (table, kind, thermo, k, v, _bound(table, k))


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_the_assimilation_flux(kind, thermo):
    """the device's pow: every element that does not take it is bit for bit"""
    _measured("assim", kind, thermo, True, dict(use_assim_flux=1, assim_flux_exponent=2.), lambda start, words: ~R.took(words, "assim"))


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_newice_type_3(kind, thermo):
    """the device's hypot: the elements with the exactly-calm nodes are bit for bit, and so is every element that forms no new ice (del_c = 0 / ... = 0)"""
    calm = _case(kind, False)[7]

    def exact(start, words):
        m = ~R.took(words, "supercooled")
        m[calm] = True
        return m
    _measured("newice3", kind, thermo, False, dict(newice_type=3), exact)


def test_the_next_step_reads_what_the_slab_wrote():
    """after slab(), the next step is bit for bit that of a second handle given the restated state, time_relaxation_damage included, through put_state"""
    from nextsim_amd import dynamics
    opts = dict(temp_dep_healing=1)
    fe, f, tri, inp, cfg, ccfg = _handle("small", True, "winton", opts, sane=True)
    ref = R.copy(inp)
    _round(fe, f, tri, ref, cfg, ccfg, True, {}, "before the step")
    assert not np.array_equal(ref["time_relaxation_damage"], inp["time_relaxation_damage"]) and not np.array_equal(ref["conc"], inp["conc"])
    fe.step(); fe.synchronize()
    p, lm = _case("small", True)[:2]
    fe2 = dynamics.FiniteElementDynamics(p)
    f2 = dict(f, **{k: ref[k] for k in R.STATE})
    fe2.set_mesh(lm); fe2.put_state(f2); fe2.set_forcing(f2)
    fe2.step(); fe2.synchronize()
    sa, sb = fe.get_state(), fe2.get_state()
    for k in sa:
        assert R.same_bits(sa[k], sb[k]).all(), k
    assert np.abs(sa["VT"]).max() > 0 and np.isfinite(sa["VT"]).all()
    fe.close(); fe2.close()


def test_a_handle_that_never_configures_the_slab_is_unchanged():
    """the traffic model and one step, bit for bit, with and without a configured slab"""
    a, *_ = _handle("small", True, sane=True, configure=False)
    b, *_ = _handle("small", True, sane=True)
    for fe in (a, b):
        fe.step(); fe.synchronize()
    assert a.traffic_model() == b.traffic_model()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert R.same_bits(sa[k], sb[k]).all(), k
    assert np.abs(sa["VT"]).max() > 0
    a.close(); b.close()


def test_call_order_and_what_is_missing():
    from nextsim_amd import dynamics
    fe, f, tri, inp, cfg, ccfg = _handle("small", True, configure=False)
    clock = R.clock()

    def refused(call, text, code=-4):
        with pytest.raises(dynamics.NxsError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))
        return True

    slab = lambda: fe.slab(DT, clock)
    fe.fluxes(); fe.column(DT)
    assert refused(slab, "before nxs_dyn_slab_configure")
    assert refused(fe.slab_rows, "before nxs_dyn_slab")
    with pytest.raises(dynamics.NxsError) as e:
        fe.slab_configure(melt_type=3)
    assert e.value.code == -1 and "OASIS" in str(e.value)
    fe.slab_configure(**cfg)
    assert refused(slab, "del_vi_tend is missing")              # nothing was put
    fe.slab_put(**{k: inp[k] for k in R.SLAB_STATE if k != "pond_volume"})
    assert refused(lambda: fe.slab(0, clock), "dt = 0", -1) and refused(lambda: fe.slab(-DT, clock), "must be positive", -1)
    assert fe.L.nxs_dyn_slab(fe.h, DT, None) == -1 and b"no clock" in fe.L.nxs_dyn_last_error(fe.h)
    fe.slab(DT, clock)                                          # neither conc_upd nor pond_volume is needed by the defaults
    assert refused(slab, "second nxs_dyn_slab without a new nxs_dyn_column")
    got, dev = fe.slab_rows(want_device=True)
    assert all(dev[k] for k in R.ROWS) and len(set(dev.values())) == len(R.ROWS)
    lib = R.hip()
    for k in ("Qa", "delS", "del_vi_rplnt_myi"):                # the device_rows pointers give what the host copies give
        a = np.empty(tri.shape[0])
        assert lib.hipMemcpy(a.ctypes.data, dev[k], a.nbytes, 2) == 0 and R.same_bits(a, got[k]).all(), k
    fe.column_rows()                                            # (the column's rows stay readable after the slab has spent them)
    fe.slab_configure(**dict(cfg, use_assim_flux=1))
    fe.fluxes(); fe.column(DT)
    assert refused(slab, "conc_upd is missing")                 # only with the assimilation flux
    assert refused(lambda: fe.slab_get(("conc_upd",)), "conc_upd was never put")
    fe.slab_put(conc_upd=inp["conc_upd"])
    fe.slab(DT, clock)
    fe.slab_configure(**dict(cfg, use_meltponds=1))
    fe.fluxes(); fe.column(DT)
    assert refused(slab, "pond_volume is missing")              # only with the ponds
    fe.slab_put(pond_volume=inp["pond_volume"])
    fe.slab(DT, clock)
    fe.slab_configure(**dict(cfg, newice_type=1))
    fe.fluxes(); fe.column(DT)
    assert refused(slab, "newice_type = 1 on a handle of the young-ice category")
    fe.slab_configure(**cfg)
    Ne = tri.shape[0]
    fe.put_coupled(conc_fsd=np.zeros((2, Ne)))                  # floe-size bins attached
    assert refused(slab, "floe-size bins are attached")
    fe.put_coupled(conc_fsd=None)
    fe.slab(DT, clock)
    # after set_mesh on a live handle: the configuration survived, the rows went with the mesh
    lm = fe.lm
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    assert refused(slab, "before nxs_dyn_column on this mesh") and refused(fe.slab_rows, "before nxs_dyn_slab")
    R.feed_flux_state(fe, inp, _case("small", True)[5])
    fe.column_set_forcing(precip=inp["precip"], snow=np.ones(Ne))
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    fe.fluxes(); fe.column(DT)
    assert refused(slab, "del_vi_tend is missing") and refused(lambda: fe.slab_get(("age",)), "age was never put")
    fe.slab_put(**{k: inp[k] for k in R.SLAB_STATE})
    fe.slab(DT, clock)
    fe.close()
    # the classic category refuses newice_type 4
    fe, f, tri, inp, cfg, ccfg = _handle("small", False, "zero_layer", dict(newice_type=4))
    fe.fluxes(); fe.column(DT)
    with pytest.raises(dynamics.NxsError) as e:
        fe.slab(DT, clock)
    assert e.value.code == -4 and "newice_type = 4 on a handle of the classic category" in str(e.value)
    fe.close()
