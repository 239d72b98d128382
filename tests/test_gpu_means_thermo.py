"""The thermodynamic Moorings means on the device (include/nxs_dyn.h: NXS_MEANS_THERMO_BEGIN ..) against tests/means_thermo_ref.py, the numpy restatement of
the cases of updateMeans (FE.cpp:8518-8924) that tests/means_ref.py does not cover, fed with the host copies of the very rows the device holds: the flux,
column and slab state and the slab's rows through the wrapper's getters, the atmosphere and the column's forcing as they were uploaded.

Tolerances: every variable without a math-library call is compared BIT FOR BIT, a NaN matching a NaN (drag_ti of an ice-free element is 0 / 0 on both sides):
acc += x * tf is a rounded product and a rounded sum on both sides, the negated five are staged as -(x * tf) and a + (-b) is a - b, the ages are a rounded
product and a rounded quotient by the same constant.
  wspeed contains hypot (windSpeedElement, FE.cpp:6359-6370), OCML's on the device against the C library's in numpy.  Its terms are non-negative, so nothing
  cancels and the bound is relative.  With u = 2^-53: each hypot is within HYPOT_RTOL of numpy's (tests/test_gpu_means.py's bound for a device hypot against
  numpy's), and so is their sum; behind it each rounding may fall differently on the two sides, <= 2 u each: the two sums of the three terms (0 + h is exact),
  the division by 3 and the product with time_factor are four per call, and over ROUNDS calls the accumulation rounds ROUNDS - 1 times (0 + x is exact), each
  relative to a partial sum that is no larger than the total.  |device - numpy| <= (HYPOT_RTOL + 2 u (4 + ROUNDS - 1)) * numpy.
"""
import functools

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import means_ref as MR
import means_thermo_ref as T
import slab_ref as R
from nextsim_amd import _abi
from test_gpu_means import HYPOT_RTOL, _same

pytestmark = pytest.mark.gpu

DT = R.DT
ROUNDS = 3
TFS = (0.25, 0.5, 0.25)                          # two different time factors over three rounds
WSPEED_RTOL = HYPOT_RTOL + 2 * 2.0 ** -53 * (4 + ROUNDS - 1)
HUM_ROW = {"dewpoint": "dair", "sphuma": "sphuma", "mixrat": "mixrat"}
HUM_ID = {"dewpoint": "d2m", "sphuma": "sphuma", "mixrat": "mixrat"}
SNOW_ID = {"precip_snowfr": "snowfr", "snowfall": "snowfall"}


@functools.lru_cache(maxsize=None)
def _case(kind, young, nparts=1, rank=0):
    gm, p, g, lms, fields = cases.make_case(kind, nparts=nparts, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)
    return (p, lms[rank], fields[rank])


def _inputs(lm, f, p):
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, _, _ = R.make_inputs(lm.coord_x, lm.coord_y, tri)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    return tri, R.sane_inputs(inp, f), finp


def valid_names(winton, hum, lw, snow):
    """every thermodynamic variable this configuration can accumulate: t1 / t2 need WINTON, of each alias group the configured source"""
    drop = {HUM_ID[h] for h in HUM_ID if h != hum} | {k for k in ("Qlw_in", "tcc") if k != lw} | {SNOW_ID[s] for s in SNOW_ID if s != snow}
    if not winton:
        drop |= {"t1", "t2"}
    return tuple(k for k in _abi.MEANS_THERMO if k not in drop)


class Rig:
    """a handle set up as tests/test_gpu_slab.py sets it up (slab_ref.gpu_handle: the designed rows bent to the case's own ice state, so that a dynamics step can
    follow), the host copies of the atmosphere and the column's forcing, and one round of the chain"""

    def __init__(self, p, lm, f, young, thermo="winton", hum="dewpoint", lw="Qlw_in", snow="precip_snowfr", stage=1):
        from nextsim_amd import dynamics
        self.p, self.young, self.winton = p, young, thermo == "winton"
        self.hum, self.lw, self.snow = hum, lw, snow
        self.design(lm, f)
        self.fe = fe = dynamics.FiniteElementDynamics(p)
        fe.set_option("means_stage", stage)
        fe.set_mesh(lm); fe.put_state(self.f); fe.set_forcing(self.f)
        fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1, humidity_source=hum, longwave_source=lw))   # (the drags stay: see slab_ref.gpu_handle)
        fe.column_configure(**CR.default_config(thermo_type=thermo, snowfall_source=snow))
        fe.slab_configure(**R.category_config(young))
        self.feed_rows()

    def design(self, lm, f):
        """the designed rows on the mesh lm, whose own fields are f"""
        self.lm = lm
        self.tri, self.inp, self.finp = _inputs(lm, f, self.p)
        inp, finp = self.inp, self.finp
        self.f = dict(f, **{k: inp[k].copy() for k in R.STATE[:-1]}, wind=inp["wind"].copy(), time_relaxation_damage=inp["time_relaxation_damage"].copy())
        snow_row = np.linspace(0.1, 0.9, lm.num_elements) if self.snow == "precip_snowfr" else 0.5 * inp["precip"]
        self.atm = dict(tair=finp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp[HUM_ROW[self.hum]], longwave=finp[self.lw])
        self.forcing = dict(precip=inp["precip"], snow=np.ascontiguousarray(snow_row), ocean_temp=inp["sst"], ocean_salt=inp["sss"], mld=inp["mld"])

    def feed_rows(self):
        """every thermodynamic row of the handle, on the mesh it has now"""
        fe, inp = self.fe, self.inp
        R.feed_flux_state(fe, inp, self.finp)
        fe.flux_set_atmosphere(**self.atm)
        fe.column_set_forcing(**self.forcing)
        fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
        fe.slab_put(**{k: inp[k] for k in _abi.SLAB_STATE})

    def chain(self, step=True):
        fe = self.fe
        fe.fluxes(); fe.column(DT); fe.slab(DT, R.clock())
        if step:
            fe.step()

    def sources(self):
        fe = self.fe
        fe.synchronize()
        st = fe.get_state()
        src = dict(conc=st["conc"], conc_young=st["conc_young"], wind=self.f["wind"])
        src.update(fe.flux_get())
        if self.winton:
            src.update(fe.column_get())
        src.update(fe.slab_get(_abi.SLAB_STATE))
        src.update(fe.slab_rows())
        src.update(self.atm); src.update(self.forcing)
        return src

    def names(self):
        return valid_names(self.winton, self.hum, self.lw, self.snow)


def _compare(names, el, ref, what):
    for k, name in enumerate(names):
        if name in T.LIBM:
            assert np.array_equal(np.isnan(el[:, k]), np.isnan(ref[:, k])), (what, name)
            ok = np.isfinite(ref[:, k]) & (ref[:, k] != 0)
            err = np.abs(el[ok, k] - ref[ok, k]) / np.abs(ref[ok, k])
            print(f"{what}: {name} max rel err {err.max():.3e} (bound {WSPEED_RTOL:.3e}), {np.count_nonzero(el[:, k] != ref[:, k])} of {el.shape[0]} values differ")
            np.testing.assert_allclose(el[:, k], ref[:, k], rtol=WSPEED_RTOL, atol=0, err_msg=f"{what}: {name}")
        else:
            bad = np.flatnonzero(~R.same_bits(el[:, k], ref[:, k]))
            assert bad.size == 0, (what, name, bad.size, bad[:5], el[bad[:3], k], ref[bad[:3], k])


def _lists(names, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(names[at:at + n]); at += n
    assert at == len(names) and all(out), (at, len(names))
    return out


# ---- parity --------------------------------------------------------------------------------------------------------------------------------------------------

# the young-ice category with WINTON (dew point, Qlw_in, precip * snowfr) and the classic category with the zero-layer column (the other alias of each group; the
# two other humidities, one per stage); the list lengths: the cap, an odd one, one, and what is left
CONFIGS = {"young-winton": (True, "winton", {1: "dewpoint", 0: "dewpoint"}, "Qlw_in", "precip_snowfr", (24, 24, 7, 1, 2)),
           "classic-zero_layer": (False, "zero_layer", {1: "mixrat", 0: "sphuma"}, "tcc", "snowfall", (24, 24, 7, 1))}


@pytest.mark.parametrize("stage", [1, 0])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_accumulation_parity_every_variable(config, stage):
    young, thermo, hums, lw, snow, sizes = CONFIGS[config]
    p, lm, f = _case("small", young)
    assert lm.local_nelements % 256 != 0          # the last workgroup has a tail
    seen = set()
    for names in _lists(valid_names(thermo == "winton", hums[stage], lw, snow), sizes):
        rig = Rig(p, lm, f, young, thermo, hums[stage], lw, snow, stage)
        rig.fe.means_configure(names)
        ref = T.ThermoMeansRef(lm.num_elements, lm.local_nelements, young, names)
        for tf in TFS:
            rig.chain()
            rig.fe.means_update(tf)
            src = rig.sources()
            ref.update(tf, src, rig.tri)
        el, nod, de, dn = rig.fe.means_get()
        assert nod is None and de and el.shape == (lm.num_elements, len(names))
        _compare(names, el, ref.el, f"{config}, stage {stage}, {len(names)} variables")
        for name in ("sst", "Qa", "fwflux", "age", "tsurf", "wspeed", "tair", "precip", "saltflux"):
            if name in names:
                assert np.nanmax(np.abs(el[:, names.index(name)])) > 0, name
        seen |= set(names)
        rig.fe.close()
    want = set(_abi.MEANS_THERMO) - ({"sphuma", "mixrat", "tcc", "snowfall"} if young else {"t1", "t2", "d2m", "Qlw_in", "snowfr", "sphuma" if stage else "mixrat"})
    assert seen == want


def test_every_new_id_is_in_some_parity_list():
    seen = set()
    for young, thermo, hums, lw, snow, sizes in CONFIGS.values():
        for hum in hums.values():
            seen |= set(valid_names(thermo == "winton", hum, lw, snow))
    assert seen == set(_abi.MEANS_THERMO)


# ---- old and new ids ---------------------------------------------------------------------------------------------------------------------------------------

def test_a_mixed_list_gives_the_columns_of_the_two_lists_apart():
    p, lm, f = _case("small", True)
    old, new = ("conc", "damage", "ice_mask", "drag_ui", "sigma_s"), ("sst", "Qa", "fwflux", "drag_ti", "tsurf", "wspeed", "age")
    mixed = ("conc", "sst", "damage", "Qa", "ice_mask", "fwflux", "drag_ui", "drag_ti", "tsurf", "sigma_s", "wspeed", "age")
    got = {}
    for key, names in (("old", old), ("new", new), ("mixed", mixed)):
        rig = Rig(p, lm, f, True)
        rig.fe.means_configure(names)
        for tf in TFS[:2]:
            rig.chain(); rig.fe.means_update(tf)
        got[key] = rig.fe.means_get()[0]
        rig.fe.close()
    for k, name in enumerate(mixed):
        apart = got["old"][:, old.index(name)] if name in old else got["new"][:, new.index(name)]
        assert _same(got["mixed"][:, k], apart), name
        assert name in old or np.nanmax(np.abs(apart)) > 0, name


@pytest.mark.parametrize("stage", [1, 0])
def test_a_list_of_old_ids_alone_gives_the_bits_it_gave(stage):
    """against means_ref.MeansRef, as tests/test_gpu_means.py compares: the kernel a list of old ids launches is the one it always launched"""
    from nextsim_amd import dynamics
    p, lm, f = _case("small", True)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_option("means_stage", stage)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.means_configure(MR.ELEMENTAL)
    ref = MR.MeansRef(lm.num_nodes, lm.num_elements, lm.local_nelements, True, MR.ELEMENTAL, ())
    for tf in TFS:
        fe.step(); fe.means_update(tf)
        fe.synchronize()
        host, _ = fe.updateIceDiagnostics()
        ref.update(tf, fe.get_state(), diag=fe.get_diag(), ice_diag=host, wind=f["wind"], drag_ui=f["drag_ui"], drag_ui_young=f["drag_ui_young"])
    el = fe.means_get()[0]
    for k, name in enumerate(MR.ELEMENTAL):
        assert _same(el[:, k], ref.el[:, k]), name
    assert np.abs(el[:, MR.ELEMENTAL.index("divergence")]).max() > 0
    fe.close()


# ---- ghosts ------------------------------------------------------------------------------------------------------------------------------------------------

def test_ghost_element_rows_stay_zero():
    p, lm, f = _case("small", True, 2, 0)
    assert 0 < lm.local_nelements < lm.num_elements and lm.local_nelements % 256 != 0
    names = ("sst", "Qa", "fwflux", "age", "drag_ti", "tsurf", "wspeed", "tair", "mld")
    for stage in (1, 0):
        rig = Rig(p, lm, f, True, stage=stage)
        rig.fe.means_configure(names)
        ref = T.ThermoMeansRef(lm.num_elements, lm.local_nelements, True, names)
        for tf in (0.5, 0.5):
            rig.chain(step=False)               # (no step: a rank of two needs its neighbour for that)
            rig.fe.means_update(tf)
            ref.update(tf, rig.sources(), rig.tri)
        el = rig.fe.means_get()[0]
        _compare(names, el, ref.el, f"partition, stage {stage}")
        assert not el[lm.local_nelements:].view(np.uint64).any()                    # +0.0 exactly, every ghost row
        assert all(np.nanmax(np.abs(el[:lm.local_nelements, k])) > 0 for k in range(len(names)))
        rig.fe.close()


# ---- after the mesh changes --------------------------------------------------------------------------------------------------------------------------------

def _refused(call, *texts, code=-4):
    from nextsim_amd import dynamics
    with pytest.raises(dynamics.NxsError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert str(e.value).split(": ", 1)[1], "no message"
    for t in texts:
        assert t in str(e.value), (t, str(e.value))
    return True


def _after_a_new_mesh(rig, names, what):
    """the accumulators are zero at the new size; means_update is refused until the rows are given and the chain has run; then it is the restatement's"""
    fe, lm = rig.fe, rig.lm
    el = fe.means_get()[0]
    assert el.shape == (lm.num_elements, len(names)) and not el.view(np.uint64).any(), what
    update = lambda: fe.means_update(1.0)
    if what == "set_mesh":
        assert _refused(update, "set_mesh and put_state")
        fe.put_state(rig.f); fe.set_forcing(rig.f)
    assert _refused(update, "sst", "never given on this mesh")
    rig.feed_rows()
    assert _refused(update, "Qa", "before the first nxs_dyn_slab")
    rig.chain()
    fe.means_update(0.5)
    ref = T.ThermoMeansRef(lm.num_elements, lm.local_nelements, rig.young, names)
    ref.update(0.5, rig.sources(), rig.tri)
    el = fe.means_get()[0]
    _compare(names, el, ref.el, "after " + what)
    assert np.abs(el[:, 1]).max() > 0


def test_after_set_mesh_the_accumulators_are_zero_and_the_rows_are_wanted_again():
    p, lm, f = _case("small", True)
    names = ("sst", "Qa", "t1", "wspeed", "age")
    rig = Rig(p, lm, f, True)
    rig.fe.means_configure(names)
    rig.chain(); rig.fe.means_update(1.0)
    assert rig.fe.means_get()[0].any()
    p2, lm2, f2 = _case("tiny", True)
    assert lm2.num_elements != lm.num_elements
    rig.fe.set_mesh(lm2)
    rig.design(lm2, f2)                          # the same handle, the designed rows of the new mesh
    _after_a_new_mesh(rig, names, "set_mesh")
    rig.fe.close()


def test_after_a_regrid_the_accumulators_are_zero_and_the_rows_are_wanted_again():
    from nextsim_amd import dynamics
    from test_gpu_regrid_handle import _fields, _global_mesh
    x, y, tri, ng = cases.rect_mesh(24, 1)
    p, lm, f = _fields(_global_mesh(x, y, tri, ng), True)
    assert lm.local_nelements % 256 != 0
    names = ("sst", "Qa", "t1", "wspeed", "age")
    rig = Rig(p, lm, f, True)
    rig.fe.means_configure(names)
    rig.chain(); rig.fe.means_update(1.0)
    assert rig.fe.means_get()[0].any()
    prev = np.arange(1, lm.num_nodes + 1, dtype=np.float64)
    info = rig.fe.regrid(lm, prev, ng, {k: rig.f[k] for k in dynamics.REGRID_INPUTS}, (), moved=(x, y))
    assert info["num_failed"] == 0
    rig.fe.set_forcing(rig.f)
    _after_a_new_mesh(rig, names, "regrid")
    rig.fe.close()


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_names_the_variable_and_the_handle_stays_usable():
    from nextsim_amd import dynamics
    p, lm, f = _case("small", True)
    tri, inp, finp = _inputs(lm, f, p)
    Ne = lm.num_elements
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    update = lambda: fe.means_update(1.0)

    def configured(*names):
        fe.means_configure(names)
        return update
    # a source row that was never put
    assert _refused(configured("sst"), "sst", "nxs_dyn_flux_put")
    assert _refused(configured("tsurf"), "tsurf") and _refused(configured("drag_ti"), "drag_ti")
    assert _refused(configured("age"), "age", "nxs_dyn_slab_put") and _refused(configured("conc_upd"), "conc_upd")
    assert _refused(configured("precip"), "precip", "nxs_dyn_column_set_forcing") and _refused(configured("tair"), "tair", "nxs_dyn_flux_set_atmosphere")
    assert _refused(configured("wspeed"), "wspeed", "forcing")
    fe.set_forcing(f)
    configured("wspeed")()
    # an alias before the configuration that says which row it is
    assert _refused(configured("d2m"), "d2m", "nxs_dyn_flux_configure") and _refused(configured("snowfr"), "snowfr", "nxs_dyn_column_configure")
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1))
    R.feed_flux_state(fe, inp, finp)
    configured("sst", "tsurf", "drag_ti", "d2m", "Qlw_in", "tair")()
    # an alias that is not the configured source
    assert _refused(configured("mixrat"), "mixrat", "the humidity row is d2m") and _refused(configured("sphuma"), "sphuma", "humidity_source")
    assert _refused(configured("tcc"), "tcc", "the long-wave row is Qlw_in")
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1, longwave_source="tcc", humidity_source="mixrat"))
    assert _refused(configured("Qlw_in"), "Qlw_in", "the long-wave row is tcc") and _refused(configured("d2m"), "d2m", "the humidity row is mixrat")
    configured("tcc", "mixrat")()
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1))
    fe.column_configure(**CR.default_config(thermo_type="winton", snowfall_source="snowfall"))
    fe.column_set_forcing(precip=inp["precip"], snow=np.ones(Ne), ocean_temp=inp["sst"], ocean_salt=inp["sss"], mld=inp["mld"])
    assert _refused(configured("snowfr"), "snowfr", "the snow row is snowfall")
    configured("snowfall", "mld", "ocean_temp", "ocean_salt", "precip")()
    fe.column_configure(**CR.default_config(thermo_type="winton", snowfall_source="precip_tair"))
    assert _refused(configured("snowfr"), "snowfr", "not read") and _refused(configured("snowfall"), "snowfall", "not read")
    fe.column_configure(**CR.default_config(thermo_type="winton"))
    assert _refused(configured("snowfall"), "snowfall", "the snow row is snowfr")
    configured("snowfr")()
    # t1 / t2 without WINTON rows: never put, or the zero-layer column
    assert _refused(configured("t1"), "t1", "WINTON") and _refused(configured("t2"), "t2", "WINTON")
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    configured("t1", "t2")()
    fe.column_configure(**CR.default_config(thermo_type="zero_layer"))
    assert _refused(configured("t2"), "t2", "WINTON")
    fe.column_configure(**CR.default_config(thermo_type="winton"))
    # a row of the slab before the first slab on this mesh
    fe.slab_configure(**R.category_config(True))
    fe.slab_put(**{k: inp[k] for k in _abi.SLAB_STATE})
    configured("age", "conc_upd", "fyi_fraction")()
    for name in ("Qa", "fwflux", "dci_mlt_myi", "saltflux"):
        assert _refused(configured(name), name, "before the first nxs_dyn_slab")
    fe.fluxes(); fe.column(DT)
    assert _refused(configured("Qa"), "Qa", "before the first nxs_dyn_slab")
    fe.slab(DT, R.clock())
    configured("Qa", "fwflux", "dci_mlt_myi", "saltflux")()
    # what the configuration refuses, and that it leaves the previous one
    fe.means_configure(("sst", "Qa"))
    fe.means_reset(); fe.means_update(1.0)
    for bad in (127, 20, 63, _abi.NXS_MEANS_THERMO_BEGIN + len(_abi.MEANS_THERMO), 255, 256, -1, _abi.MEANS_ID["VT_x"]):
        assert _refused(lambda: fe.means_configure(["sst", bad]), "elemental_ids[1]", code=-1), bad
    assert _refused(lambda: fe.means_configure([], ["sst"]), code=-1)            # a thermodynamic id in the nodal list
    assert _refused(lambda: fe.means_configure([("sst", True)]), "ICE_MASK", code=-1)
    assert _refused(lambda: fe.means_configure(["sst"] * 25), code=-1)
    el = fe.means_get()[0]
    assert el.shape == (Ne, 2) and np.array_equal(el[:lm.local_nelements, 0], fe.flux_get(("sst",))["sst"][:lm.local_nelements] * 1.0)
    # still a working handle: a mask on a thermodynamic variable, a step, an update
    fe.means_configure([("sst", True), "ice_mask", "Qa"])
    fe.step(); fe.means_update(1.0); fe.synchronize()
    assert fe.means_get()[0].any()
    fe.close()


# ---- no side effects -----------------------------------------------------------------------------------------------------------------------------------------

def test_means_update_changes_no_state_row_and_no_thermodynamic_row():
    p, lm, f = _case("small", True)
    rig = Rig(p, lm, f, True)
    rig.chain()
    fe = rig.fe
    names = rig.names()

    def everything():
        fe.synchronize()
        out = {"state:" + k: v for k, v in fe.get_state().items()}
        out.update({"flux:" + k: v for k, v in fe.flux_get().items()})
        out.update({"column:" + k: v for k, v in fe.column_get().items()})
        out.update({"slab:" + k: v for k, v in fe.slab_get().items()})
        out.update({"slab row:" + k: v for k, v in fe.slab_rows().items()})
        out.update({"flux row:" + k: v for k, v in fe.fluxes_get().items()})
        out.update({"column row:" + k: v for k, v in fe.column_rows().items()})
        return out
    before = everything()
    for at in range(0, len(names), 24):
        fe.means_configure(names[at:at + 24])
        for stage in (1, 0):
            fe.set_option("means_stage", stage)
            fe.means_update(0.5)
    after = everything()
    assert before.keys() == after.keys() and len(before) > 100
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    fe.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------------------

def test_a_time_mean_moorings_record_with_thermodynamic_variables(tmp_path):
    from nextsim_amd import io
    p, lm, f = _case("small", True)
    rig = Rig(p, lm, f, True)
    fe = rig.fe
    names = ("sst", "Qa", "fwflux", "ice_mask")
    fe.means_configure(names, ["VT_x"])
    ref = T.ThermoMeansRef(lm.num_elements, lm.local_nelements, True, names[:3])
    for tf in (0.5, 0.5):
        rig.chain(); fe.means_update(tf)
        ref.update(tf, rig.sources())
    el = fe.means_get()[0]
    _compare(names[:3], el[:, :3], ref.el, "before the record")
    ncols, nrows = 40, 30
    spacing = np.ptp(lm.coord_x) / (ncols - 1)
    lon = np.zeros((nrows, ncols), np.float32); lat = np.zeros((nrows, ncols), np.float32)
    path = str(tmp_path / "Moorings.nc")
    var = [dict(name=n, standard_name=n, long_name=n, units="1", cell_methods="area: mean") for n in ("sst", "hfs", "wfo", "ice_mask", "siu")]
    io.moorings_create(path, lon, lat, var, format=io.NC_CLASSIC)
    ge, gn = io.moorings_append_means(path, 1.0, fe, lm.coord_x.min(), lm.coord_y.max(), spacing, ncols, nrows)
    assert ge.shape == (4, ncols * nrows) and gn.shape == (1, ncols * nrows)
    inside = ge[3] > 0
    assert inside.any() and all(np.nanmax(np.abs(ge[k][inside])) > 0 for k in range(3))
    # the grid holds the mesh means: every sampled value lies within the range of its column
    for k in range(3):
        assert np.nanmin(ge[k][inside]) >= np.nanmin(el[:, k]) and np.nanmax(ge[k][inside]) <= np.nanmax(el[:, k]), names[k]
    assert not fe.means_get()[0].any()             # resetMeshMean followed the record
    assert io.moorings_file_format(path) == io.NC_CLASSIC
    fe.close()
