"""nxs_dyn_regrid with the thermodynamic state carried across on the device (nxs_dyn_regrid_carry_thermo): the rows of nxs_dyn_flux_state, nxs_dyn_column_state and
nxs_dyn_slab_state as columns of the regrid, against the host chain of tests/regrid_ref.py with the same rows handed in as `extras` with the kinds and bounds of
dynamics.REGRID_THERMO_COLUMNS (model/model_variable.cpp).

Expected agreement: BITWISE, every row -- the carried columns go through the kernels the caller's extras go through (tests/test_gpu_regrid_handle.py), and the
conservative remapping treats every column alike.  The three re-made rows are constants."""
import functools

import numpy as np
import pytest

import cases
import regrid_ref as R
import slab_ref as SR
from nextsim_amd import _abi, dynamics
from test_gpu_regrid_handle import MU, _eq, _fields, _global_mesh, _interp, _pair, _remap

pytestmark = pytest.mark.gpu

DRAG_ICE_T = 1.25e-3
REMADE = sum(1 << _abi.FLUX_STATE.index(k) for k in dynamics.REGRID_THERMO_REMADE)
T_NOICE = -MU * R.SI


def _mask(names, rows):
    return sum(1 << rows.index(k) for k in names if k in rows)


def _thermo_rows(rng, st, cx):
    """Every row of the three state structs on the old mesh.  tice1 / tice2 are negative everywhere (the enthalpy transformation divides by the temperature);
    conc_upd, freeze_days and fyi_fraction lie outside their bounds on the eastern third of the box, so that after the remapping whole new triangles still do."""
    Ne = st["thick"].size
    east = cx > cx.min() + 0.66 * np.ptp(cx)
    assert east.any() and not east.all()
    tice = lambda: np.where(st["thick"] > 0, rng.uniform(-30., -0.5, Ne), T_NOICE)   # noqa: E731
    rows = dict(tice0=rng.uniform(-30., -0.5, Ne), tsurf_young=rng.uniform(-20., 0., Ne), sst=rng.uniform(-1.8, 5., Ne), sss=rng.uniform(28., 35., Ne),
                drag_ti=rng.uniform(1e-3, 2e-3, Ne), drag_ti_young=rng.uniform(1e-3, 2e-3, Ne), pond_fraction=rng.uniform(0.01, 0.3, Ne),
                lid_volume=rng.uniform(0., 0.01, Ne), tice1=tice(), tice2=tice(),
                conc_upd=np.where(east, 1.3, rng.uniform(-1.4, 0.5, Ne)), pond_volume=rng.uniform(0., 0.05, Ne), del_vi_tend=rng.normal(0., 0.01, Ne),
                freeze_days=np.where(east, -3., rng.uniform(0., 200., Ne)), freeze_onset=rng.uniform(0., 1., Ne), conc_summer=rng.uniform(0., 1., Ne),
                thick_summer=rng.uniform(0., 3., Ne), fyi_fraction=np.where(east, 1.2, rng.uniform(0., 1., Ne)), age_det=rng.uniform(0., 3e7, Ne),
                age=rng.uniform(0., 3e7, Ne))
    assert (rows["tice1"] < 0).all() and (rows["tice2"] < 0).all()
    assert (rows["conc_upd"] > 1).any() and (rows["conc_upd"] < -1).any() and (rows["freeze_days"] < 0).any() and (rows["fyi_fraction"] > 1).any()
    return {k: np.ascontiguousarray(v) for k, v in rows.items()}


def _as_extras(rows):
    """the rows present, as the chain's extras: kinds and bounds of the table, in its order"""
    names = [c[0] for c in dynamics.REGRID_THERMO_COLUMNS if c[0] in rows]
    ex = []
    for name, kind, lo, hi, is_tice in dynamics.REGRID_THERMO_COLUMNS:
        if name in rows:
            x = dict(old=rows[name], transformation=kind, is_tice=is_tice)
            if lo is not None:
                x["min"] = lo
            if hi is not None:
                x["max"] = hi
            ex.append(x)
    return names, ex


def _put(fe, rows):
    flux = {k: rows[k] for k in _abi.FLUX_STATE if k in rows}
    col = {k: rows[k] for k in _abi.COL_STATE if k in rows}
    slab = {k: rows[k] for k in _abi.SLAB_STATE if k in rows}
    if flux:
        fe.flux_put(**flux)
    if col:
        fe.column_put(**col)
    if slab:
        fe.slab_put(**slab)


def _present(fe):
    """the rows the getters hand out on the handle's mesh, one by one; a missing row is NXS_ERR_STATE"""
    out = {}
    for names, get in ((_abi.FLUX_STATE, fe.flux_get), (_abi.COL_STATE, fe.column_get), (_abi.SLAB_STATE, fe.slab_get)):
        for k in names:
            try:
                out[k] = get((k,))[k]
            except dynamics.NxsError as e:
                assert e.code == -4 and k in str(e), str(e)
    return out


@functools.lru_cache(maxsize=None)
def _run(pair, young=True, winton=True, mode="carry", coupled=False, tile=1):
    """2 steps on the old mesh, the thermodynamic rows put, then nxs_dyn_regrid and the host chain on the same inputs.
    mode: "carry" (the new call), "extras" (carry off, the same rows as the caller's host extras), "off" (no call at all), "off_again" (carry = 1, then 0),
    "flux_only" (carry on, only nxs_dyn_flux_state put)."""
    xo, yo, to, xn, yn, tn, prev, ng = _pair(pair)
    gm, gm2 = _global_mesh(xo, yo, to, ng), _global_mesh(xn, yn, tn, ng)
    p, lm, f = _fields(gm, young)
    _, lm2, f2 = _fields(gm2, young)
    Ne, Nn = lm.num_elements, lm.num_nodes
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_option("regrid_tile", tile)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    cp = None
    if coupled:
        rc = np.random.default_rng(12)
        fe.put_coupled(cum_damage=rc.uniform(0., 0.2, Ne), conc_fsd=np.ascontiguousarray(rc.dirichlet([1., 1., 1.], Ne).T * f["conc"]))
    for _ in range(2):
        fe.step()
    fe.synchronize()
    st = fe.get_state()
    if coupled:
        cp = fe.get_coupled(True, 3)
    assert (st["thick"] == 0.).any() and np.abs(st["UM"]).max() > 0.
    xm, ym = lm.coord_x + st["UM"][:Nn], lm.coord_y + st["UM"][Nn:]
    rows = _thermo_rows(np.random.default_rng(31), st, xo[to].mean(1))
    if not winton:
        rows = {k: v for k, v in rows.items() if k not in _abi.COL_STATE}
    if mode == "flux_only":
        rows = {k: v for k, v in rows.items() if k in _abi.FLUX_STATE}
    names, extras = _as_extras(rows)
    ref, ref_rows, nb_var = R.chain(st, (to, xm, ym), (tn, xn, yn), prev, ng, young, _remap, _interp, extras, cp, MU)
    ref_rows = dict(zip(names, ref_rows))
    given = ()
    if mode == "extras":
        given = [dict(x) for x in extras]
    else:
        _put(fe, rows)
    if mode in ("carry", "flux_only", "off_again"):
        fe.regrid_carry_thermo(carry=True, drag_ice_t=DRAG_ICE_T)
    if mode == "off_again":
        fe.regrid_carry_thermo(carry=False)
    info = fe.regrid(lm2, prev, ng, {k: f2[k] for k in dynamics.REGRID_INPUTS}, given, moved=(xm, ym), freezingpoint_mu=MU)
    out = dict(info=info, tinfo=fe.regrid_thermo_info(), got=fe.get_state(), ref=ref, ref_rows=ref_rows, nb_var=nb_var, names=names,
               got_rows=dict(zip(names, (x["new"] for x in given))) if mode == "extras" else _present(fe),
               got_coupled=fe.get_coupled(True, 3) if coupled else None)
    fe.close()
    return out


def _assert_preconditions(r):
    """on the chain's output: ice-free new triangles, and every clamp and the no-ice rule have triangles to bite on"""
    ref, rr = r["ref"], r["ref_rows"]
    assert (ref["thick"] == 0.).any() and (ref["thick"] > 0.).any()
    assert (rr["conc_upd"] == 1.).any() and (rr["freeze_days"] == 0.).any() and (rr["fyi_fraction"] == 1.).any()
    assert rr["conc_upd"].min() >= -1. and rr["conc_upd"].max() <= 1. and rr["freeze_days"].min() >= 0. and rr["fyi_fraction"].max() <= 1.


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair,young,winton", [("rect", True, True), ("golden", True, True), ("rect", False, False)])
def test_carried_rows_are_the_chains_bits(pair, young, winton):
    r, plain = _run(pair, young, winton, "carry"), _run(pair, young, winton, "extras")
    _assert_preconditions(r)
    carried = [c[0] for c in dynamics.REGRID_THERMO_COLUMNS if winton or c[0] not in _abi.COL_STATE]
    assert r["names"] == carried and len(carried) == (17 if winton else 15)
    for k in carried:
        assert _eq(r["got_rows"][k], r["ref_rows"][k]), k
    assert set(r["got_rows"]) == set(carried) | set(dynamics.REGRID_THERMO_REMADE)
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:      # more columns, the same state: against the chain and against the regrid without carry
        assert _eq(r["got"][k], r["ref"][k]), k
        assert _eq(r["got"][k], plain["got"][k]), k
    t = r["tinfo"]
    assert t["flux_carried"] == _mask(carried, _abi.FLUX_STATE) == 0x8f and t["flux_remade"] == REMADE == 0x70
    assert t["col_carried"] == (3 if winton else 0) and t["slab_carried"] == (1 << len(_abi.SLAB_STATE)) - 1
    assert t["nb_var_element"] == r["info"]["nb_var_element"] == r["nb_var"] == 13 + len(carried) and t["tiled"] == 0
    assert t["flux_remade_names"] == dynamics.REGRID_THERMO_REMADE and r["info"]["num_failed"] == 0


# ---- 2. the library against itself -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["rect", "golden"])
def test_carry_gives_the_bits_of_the_same_rows_as_host_extras(pair):
    r, plain = _run(pair, True, True, "carry"), _run(pair, True, True, "extras")
    assert plain["tinfo"]["flux_carried"] == plain["tinfo"]["col_carried"] == plain["tinfo"]["slab_carried"] == plain["tinfo"]["flux_remade"] == 0
    assert plain["info"]["nb_var_element"] == r["info"]["nb_var_element"] == 30
    for k in r["names"]:
        assert _eq(r["got_rows"][k], plain["got_rows"][k]), k


# ---- 3. the re-made rows and the no-ice rule -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["rect", "golden"])
def test_remade_rows_and_the_ice_temperatures_without_ice(pair):
    r = _run(pair, True, True, "carry")
    rows, Ne2 = r["got_rows"], r["got"]["thick"].size
    assert _eq(rows["drag_ti"], np.full(Ne2, DRAG_ICE_T)) and _eq(rows["drag_ti_young"], np.full(Ne2, DRAG_ICE_T))
    assert _eq(rows["pond_fraction"], np.zeros(Ne2))
    no_ice = r["got"]["thick"] == 0.
    assert no_ice.any() and not no_ice.all()
    for k in ("tice1", "tice2"):
        assert _eq(rows[k][no_ice], np.full(no_ice.sum(), T_NOICE)), k
        assert (rows[k][~no_ice] != T_NOICE).any(), k


# ---- 4. partial state ------------------------------------------------------------------------------------------------------------------------

def test_only_the_rows_that_were_put_are_carried():
    r = _run("rect", True, True, "flux_only")
    t = r["tinfo"]
    assert t["slab_carried"] == 0 and t["col_carried"] == 0 and t["flux_carried"] == 0x8f and t["flux_remade"] == 0x70 and t["nb_var_element"] == 13 + 5
    assert set(r["got_rows"]) == set(_abi.FLUX_STATE)                   # slab_get and column_get answered NXS_ERR_STATE for every row (_present)
    for k in r["names"]:
        assert _eq(r["got_rows"][k], r["ref_rows"][k]), k
    assert _eq(r["got_rows"]["drag_ti"], np.full(r["got"]["thick"].size, DRAG_ICE_T))


# ---- 5. off by default, and off again --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["off", "off_again"])
def test_without_the_call_every_row_is_missing_as_before(mode):
    r = _run("rect", True, True, mode)
    assert r["got_rows"] == {}
    t = r["tinfo"]
    assert t["flux_carried"] == t["col_carried"] == t["slab_carried"] == t["flux_remade"] == 0 and t["nb_var_element"] == r["info"]["nb_var_element"] == 13
    for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
        assert _eq(r["got"][k], r["ref"][k]), k


# ---- 6. the run continues --------------------------------------------------------------------------------------------------------------------

def _everything(fe):
    fe.synchronize()
    out = {"state:" + k: v for k, v in fe.get_state().items()}
    out.update({"flux:" + k: v for k, v in fe.flux_get().items()})
    out.update({"column:" + k: v for k, v in fe.column_get().items()})
    out.update({"slab:" + k: v for k, v in fe.slab_get().items()})
    out.update({"slab row:" + k: v for k, v in fe.slab_rows().items()})
    return out


def test_the_thermodynamic_run_continues():
    """fluxes -> column -> slab -> step on the new mesh after a carried regrid, against a fresh handle on the new mesh that was given the chain's output"""
    from test_gpu_means_thermo import DT, Rig
    xo, yo, to, xn, yn, tn, prev, ng = _pair("golden")
    p, lm, f = _fields(_global_mesh(xo, yo, to, ng), True)
    _, lm2, f2 = _fields(_global_mesh(xn, yn, tn, ng), True)
    Nn = lm.num_nodes
    rig = Rig(p, lm, f, True)
    fe = rig.fe
    fe.column_put(tice1=np.minimum(rig.inp["tice1"], -0.01), tice2=np.minimum(rig.inp["tice2"], -0.01))
    rig.chain()                                        # (the old mesh has run its chain: every done flag is up, every output row exists)
    fe.synchronize()
    st = fe.get_state()
    rows = dict(fe.flux_get(), **fe.column_get(), **fe.slab_get(_abi.SLAB_STATE))
    assert (rows["tice1"] < 0).all() and (rows["tice2"] < 0).all() and (st["thick"] == 0.).any()
    xm, ym = lm.coord_x + st["UM"][:Nn], lm.coord_y + st["UM"][Nn:]
    names, extras = _as_extras(rows)
    ref, ref_rows, nb_var = R.chain(st, (to, xm, ym), (tn, xn, yn), prev, ng, True, _remap, _interp, extras, None, MU)
    ref_rows = dict(zip(names, ref_rows))
    assert (ref["thick"] == 0.).any() and nb_var == 30

    fresh = Rig(p, lm2, f2, True)                      # the designed forcing of the new mesh; its state rows are replaced by the chain's below
    inputs = {k: fresh.f[k] for k in dynamics.REGRID_INPUTS}
    fe.regrid_carry_thermo(carry=True, drag_ice_t=DRAG_ICE_T)
    info = fe.regrid(lm2, prev, ng, inputs, (), moved=(xm, ym), freezingpoint_mu=MU)
    assert info["num_failed"] == 0 and info["nb_var_element"] == 30
    for get in (fe.fluxes_get, fe.column_rows, fe.slab_rows):          # the output rows are gone, the done flags down
        with pytest.raises(dynamics.NxsError) as e:
            get()
        assert e.value.code == -4
    with pytest.raises(dynamics.NxsError) as e:                        # ... and so is the forcing: the atmosphere is the host's to give again
        fe.fluxes()
    assert e.value.code == -4
    fe.set_forcing(fresh.f)
    with pytest.raises(dynamics.NxsError) as e:
        fe.fluxes()
    assert e.value.code == -4 and "atmosphere" in str(e.value)
    fe.flux_set_atmosphere(**fresh.atm); fe.column_set_forcing(**fresh.forcing)

    Ne2 = lm2.num_elements
    g = fresh.fe
    g.put_state(dict(fresh.f, **{k: ref[k] for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL}, **inputs)); g.set_forcing(fresh.f)
    _put(g, dict(ref_rows, drag_ti=np.full(Ne2, DRAG_ICE_T), drag_ti_young=np.full(Ne2, DRAG_ICE_T), pond_fraction=np.zeros(Ne2)))
    for h in (fe, g):
        for _ in range(2):
            h.fluxes(); h.column(DT); h.slab(DT, SR.clock()); h.step()
    a, b = _everything(fe), _everything(g)
    assert a.keys() == b.keys() and len(a) > 60
    for k in a:
        assert _eq(a[k], b[k]), k
    assert np.abs(a["state:UM"]).max() > 0. and not _eq(a["flux:sst"], ref_rows["sst"])
    rig.fe.close(); fresh.fe.close()


# ---- 7. the means see the carried rows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("carry", [True, False])
def test_means_update_after_a_regrid_names_only_what_is_missing(carry):
    from test_gpu_means_thermo import Rig
    x, y, tri, ng = cases.rect_mesh(24, 1)
    p, lm, f = _fields(_global_mesh(x, y, tri, ng), True)
    rig = Rig(p, lm, f, True)
    fe = rig.fe
    fe.column_put(tice1=np.minimum(rig.inp["tice1"], -0.01), tice2=np.minimum(rig.inp["tice2"], -0.01))
    fe.means_configure(("sst", "Qa"))
    rig.chain(); fe.means_update(1.0)
    if carry:
        fe.regrid_carry_thermo(carry=True, drag_ice_t=DRAG_ICE_T)
    prev = np.arange(1, lm.num_nodes + 1, dtype=np.float64)
    info = fe.regrid(lm, prev, ng, {k: rig.f[k] for k in dynamics.REGRID_INPUTS}, (), moved=(x, y))
    assert info["num_failed"] == 0
    fe.set_forcing(rig.f)
    with pytest.raises(dynamics.NxsError) as e:
        fe.means_update(1.0)
    assert e.value.code == -4
    if carry:                                          # sst is there: only the slab's diagnostic is wanted
        assert "Qa" in str(e.value) and "before the first nxs_dyn_slab" in str(e.value) and "never given" not in str(e.value)
        fe.flux_set_atmosphere(**rig.atm); fe.column_set_forcing(**rig.forcing)
        rig.chain(); fe.means_update(0.5); fe.synchronize()
        el = fe.means_get()[0]
        assert el.shape == (lm.num_elements, 2) and np.nanmax(np.abs(el[:, 0])) > 0 and np.nanmax(np.abs(el[:, 1])) > 0
    else:                                              # as tests/test_gpu_means_thermo.py sees it
        assert "sst" in str(e.value) and "never given on this mesh" in str(e.value)
    fe.close()


# ---- 8. a refused call leaves the thermodynamic rows alone -----------------------------------------------------------------------------------

def test_failure_leaves_the_thermodynamic_rows_alone():
    xo, yo, to, xn, yn, tn, prev, ng = _pair("rect")
    p, lm, f = _fields(_global_mesh(xo, yo, to, ng), True)
    _, lm2, f2 = _fields(_global_mesh(xn, yn, tn, ng), True)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.step(); fe.synchronize()
    rows = _thermo_rows(np.random.default_rng(31), fe.get_state(), xo[to].mean(1))
    _put(fe, rows)
    fe.regrid_carry_thermo(carry=True, drag_ice_t=DRAG_ICE_T)
    before = _present(fe)
    assert set(before) == set(rows)
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    bad = [dict(old=np.zeros(lm.num_elements), transformation=7)]
    with pytest.raises(dynamics.NxsError) as e:
        fe.regrid(lm2, prev, ng, inputs, bad, moved=(xo, yo), validate=False)
    assert e.value.code == -1 and "transformation 7" in str(e.value)
    with pytest.raises(dynamics.NxsError) as e:
        fe.regrid(lm2, prev, ng, inputs, (), validate=False)
    assert e.value.code == -1 and "moved" in str(e.value)
    # a freezingpoint_mu that is not the column configuration's
    fe.column_configure(freezingpoint_mu=0.0625)
    with pytest.raises(dynamics.NxsError) as e:
        fe.regrid(lm2, prev, ng, inputs, (), moved=(xo, yo), freezingpoint_mu=MU)
    assert e.value.code == -1 and "0.055" in str(e.value) and "0.0625" in str(e.value)
    assert fe.lm is lm
    after = _present(fe)
    assert set(after) == set(before)
    for k in before:
        assert _eq(after[k], before[k]), k
    # with carry off the two values may differ, as they always could
    fe.regrid_carry_thermo(carry=False)
    info = fe.regrid(lm2, prev, ng, inputs, (), moved=(xo, yo), freezingpoint_mu=MU)
    assert info["nb_var_element"] == 13 and _present(fe) == {}
    fe.close()


# ---- 9. rows wider than the staging tile -----------------------------------------------------------------------------------------------------

def test_wide_rows_in_column_tiles_give_the_bits_of_the_global_walk():
    """13 + cum_damage + 3 bins + 17 thermodynamic rows = 34 columns: one full tile of 31 and a tail of 3"""
    tiled, walk = _run("rect", True, True, "carry", True, 1), _run("rect", True, True, "carry", True, 0)
    _assert_preconditions(tiled)
    assert tiled["tinfo"]["tiled"] == 1 and walk["tinfo"]["tiled"] == 0
    for r in (tiled, walk):
        assert r["info"]["nb_var_element"] == r["nb_var"] == r["tinfo"]["nb_var_element"] == 34 and r["info"]["num_failed"] == 0
        for k in _abi.STATE_ELEMENT + _abi.STATE_NODAL:
            assert _eq(r["got"][k], r["ref"][k]), k
        for k in r["names"]:
            assert _eq(r["got_rows"][k], r["ref_rows"][k]), k
        assert _eq(r["got_coupled"]["cum_damage"], r["ref"]["cum_damage"])
        assert _eq(r["got_coupled"]["conc_fsd"], np.stack([r["ref"][f"conc_fsd{b}"] for b in range(3)]))
        assert _eq(r["got_rows"]["drag_ti"], np.full(r["got"]["thick"].size, DRAG_ICE_T))
    for k in tiled["got_rows"]:
        assert _eq(tiled["got_rows"][k], walk["got_rows"][k]), k
    for k in tiled["got"]:
        assert _eq(tiled["got"][k], walk["got"][k]), k
