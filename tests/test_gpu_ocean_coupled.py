"""A coupled ocean on the device (include/nxs_dyn.h: nxs_dyn_ocean_coupled_*; include/nxs_interp.h: nxs_gridmap_receive_rows) against tests/ocean_coupled_ref.py,
the line-by-line restatement.  Every bar is BIT FOR BIT, NaNs equal by position: no statement of the feature calls libm, and the build is uncontracted.
  - the receive kernel: on every golden case of tests/golden/bamg_grid_remap.npz (the real bamg's lists), for 1, 3 and 5 variables, host and device pointers,
    both ways of reading the lists, it equals the restatement on export()'s lists AND nxs_gridmap_grid_to_mesh on the interleaved, transformed input followed by
    factor * x + bias; maps restricted to 1, 255, 256 and 257 triangles;
  - the three guarded statements through nxs_dyn_ocean_coupled_put_rows (no grid involved): the fluxes' Qow from the device's OWN rows (so the fluxes' libm
    tolerance does not enter), the column, the slab with and without floe-size bins -- fed through the device_rows doors as tests/test_gpu_column.py and
    tests/test_gpu_slab.py do --, three rounds with fresh received rows each;
  - end to end on the toy mesh: receive of device fields through the mesh's own map, then fluxes -> column -> slab;
  - the life cycle and the refusals."""
import ctypes as C

import numpy as np
import pytest

import column_ref as CR
import fluxes_ref as FR
import fsd_ref as FS
import grid_remap_ref as G
import ocean_coupled_ref as OC
import slab_fsd_ref as SFR
import slab_ref as SR
import test_gpu_column as TC
import test_gpu_fsd as TF
import test_gpu_grid_remap as TG
import test_gpu_slab as TS
import test_gpu_slab_fsd as TSF
from nextsim_amd import _abi

pytestmark = pytest.mark.gpu

DT = SR.DT
ALB = FR.default_config()["ocean_albedo"]
INVALID, STATE = -1, -4
THREE = ("ocean_temp", "ocean_salt", "qsrml")


def _same(a, b):
    return G.same_bits(a, b)


def _refused(call, code, *words):
    from nextsim_amd import dynamics
    with pytest.raises(dynamics.NxsError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return True


# ---- the receive kernel ---------------------------------------------------------------------------------------------------------------------------------------

def _receive_every_way(gm, lists, G_size, what):
    from nextsim_amd import interp
    nels = lists["nels"]
    for n_var in (1, 3, 5):
        fields, a, b, factor, bias = OC.awkward_fields(G_size, n_var)
        want = OC.receive(lists, fields, a, b, factor, bias)
        x = gm.grid_to_mesh(OC.interleaved(fields, a, b))                      # [nels][n_var]
        with np.errstate(all="ignore"):
            assert _same(want, (factor[None, :] * x + bias[None, :]).T), (what, n_var, "the restatement against the interleaved application")
        d_in = [TG.Dev((G_size,), f) for f in fields]
        d_out = [TG.Dev((nels,)) for _ in fields]
        for mode in (0, 1):
            interp.gridmap_debug_receive_lists(mode)
            try:
                assert _same(gm.receive_rows(fields, a, b, factor, bias), want), (what, n_var, mode, "host -> host")
                assert _same(gm.receive_rows([d.p.value for d in d_in], a, b, factor, bias, in_device=True), want), (what, n_var, mode, "device -> host")
                assert gm.receive_rows(fields, a, b, factor, bias, out_device=[d.p.value for d in d_out]) is None
                assert _same(np.stack([d.get() for d in d_out]), want), (what, n_var, mode, "host -> device")
                for d in d_out:
                    assert d.L.hipMemcpy(d.p, np.zeros(nels).ctypes.data, nels * 8, TG.H2D) == 0
                gm.receive_rows([d.p.value for d in d_in], a, b, factor, bias, in_device=True, out_device=[d.p.value for d in d_out])
                assert _same(np.stack([d.get() for d in d_out]), want), (what, n_var, mode, "device -> device")
            finally:
                interp.gridmap_debug_receive_lists(1)                      # (the default)
        for d in d_in + d_out:
            d.free()
    return want


@pytest.mark.parametrize("name", G.CASES)
def test_receive_rows_on_every_golden_case(name):
    c, rg, gm = TG._case_map(name)
    e = gm.export()
    TG._lists_equal(e, c)
    want = _receive_every_way(gm, e, c["gridX"].size, name)                    # (the five-variable result)
    touched = np.zeros(e["nels"], bool); touched[e["tris"]] = True
    assert np.isnan(want[:, ~touched]).all()
    if name == "all_land":
        assert np.isnan(gm.receive_rows([np.ones(c["gridX"].size)])).all()
    if name == "one_cell":                                                     # entry by entry: every touched triangle holds the one cell's value
        f, a, b, factor, bias = np.array([3.25]), 2., 0.5, 0.75, -1.
        got = gm.receive_rows([f], a, b, factor, bias)[0]
        for k, t in enumerate(e["tris"]):
            assert got[t] == factor * ((0. + (f[0] * a + b) * e["w"][k]) * (1. / (0. + e["w"][k]))) + bias, (k, t)
        assert np.isnan(got[~touched]).all() and touched.sum() == e["tris"].size == 52
    # unit coefficients give the real bamg's own outputs, up to the sign of zero
    got = gm.receive_rows([c["g2m_in7"][:, v] for v in range(5)])
    assert _same(got + 0., c["g2m_out7"][:, :5].T + 0.)
    gm.close(); rg.close()


@pytest.mark.parametrize("n_tri", [1, 255, 256, 257])
def test_receive_rows_at_the_launch_edges(n_tri):
    """maps of 1, 255, 256 and 257 triangles: one thread, a block short of one lane, a full block, a block and one lane.  The mesh is `long_rows` (2496
    triangles), the only golden mesh with more than 257 -- `fine` has 96 --; the triangles kept are the first n_tri that a wet cell touches, so that the rows hold
    numbers and not NaNs alone."""
    c, rg, gm = TG._case_map("long_rows")
    nels = c["tri"].shape[0]
    touched = np.unique(c["tris"])
    assert nels > 257 and touched.size >= 257
    local = np.full(nels, -1, np.int32)
    local[touched[:n_tri]] = np.arange(n_tri)
    r = gm.restrict(local, n_tri)
    e = r.export()
    assert e["nels"] == n_tri and r.info()["nels"] == n_tri and np.unique(e["tris"]).size == n_tri
    want = _receive_every_way(r, e, c["gridX"].size, f"long_rows restricted to {n_tri}")
    assert not np.isnan(want[1]).any()
    r.close(); gm.close(); rg.close()


def test_receive_rows_argument_checks():
    from nextsim_amd.interp import NxsError
    c, rg, gm = TG._case_map("one_cell")
    for bad in ([], [np.ones(1)] * 6):
        with pytest.raises(NxsError) as e:
            gm.receive_rows(bad)
        assert e.value.code == INVALID and "n_var" in str(e.value)
    with pytest.raises(ValueError):
        gm.receive_rows([np.ones(c["gridX"].size + 1)])
    gm.close(); rg.close()


# ---- the three guards through put_rows ------------------------------------------------------------------------------------------------------------------------

def _attach_three(fe, rec):
    fe.ocean_coupled_attach(None, rows=THREE)
    fe.ocean_coupled_put_rows(**{k: rec[k] for k in THREE})


def test_fluxes_take_the_absorbed_share_of_the_short_wave():
    cfg = CR.default_config(freezingpoint_type="unesco")
    fe, p, lm, f, tri, inp, calm = TC._handle("toy", True, cfg)
    twin, *_ = TC._handle("toy", True, cfg)
    rec = OC.received_rows(inp)
    _attach_three(fe, rec)
    fe.fluxes(); twin.fluxes()
    got, base = fe.fluxes_get(), twin.fluxes_get()
    assert _same(got["Qow"], OC.qow(got, rec["qsrml"]))                       # from the device's OWN rows
    assert not _same(got["Qow"], base["Qow"]) and _same(base["Qow"], OC.qow(base, None, drop=("qsw_kept",)))
    for k in _abi.FLUX_ROWS:
        assert k == "Qow" or _same(got[k], base[k]), k                         # the other 24 rows, Qsw_ow (the TOTAL short wave) among them
    sa, sb = fe.get_state(), twin.get_state()
    for k in sa:                                                               # (the drags the fluxes update in place among them)
        assert _same(sa[k], sb[k]), k
    # detached: the un-attached bits again
    fe.ocean_coupled_detach()
    fe.fluxes()
    assert _same(fe.fluxes_get(("Qow",))["Qow"], base["Qow"])
    fe.close(); twin.close()


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
def test_column_resets_sst_and_sss_before_the_heat_flux(thermo, young):
    cfg = CR.default_config(thermo_type=thermo, freezingpoint_type="unesco", ocean_type="nudged")   # (the configured ocean_type is not consulted)
    fe, p, lm, f, tri, inp, calm = TC._handle("toy", young, cfg)
    assert lm.num_elements == 2368
    ref = CR.copy(inp)
    for call in range(3):                                                      # fresh received rows each round; the temperatures of one round feed the next
        rec = OC.received_rows(inp, seed=30 + call)
        ref.update(ocean_temp=rec["ocean_temp"], ocean_salt=rec["ocean_salt"])
        if call == 0:
            _attach_three(fe, rec)
        else:
            fe.ocean_coupled_put_rows(**{k: rec[k] for k in THREE})
        TC._fluxes_then_feed(fe, ref, young)
        fe.column(DT)
        got = fe.column_rows()
        rows, _ = OC.column(ref, cfg, tri, young, DT)
        st = dict(TC._device_state(fe, young), **fe.flux_get(("sst", "sss")))
        for k in CR.ROWS:
            bad = np.flatnonzero(~SR.same_bits(got[k], rows[k]))
            assert bad.size == 0, (thermo, young, call, k, bad[:5], got[k][bad[:3]], rows[k][bad[:3]])
        for k in CR.IN_PLACE + ("sst", "sss"):
            assert _same(st[k], ref[k]), (thermo, young, call, "state", k)
        assert _same(st["sst"], rec["ocean_temp"]) and _same(st["sss"], rec["ocean_salt"])
        assert not got["Qdw"].any() and not got["Fdw"].any() and np.abs(got["Qio"]).max() > 0
    fe.close()


def _slab_round(fe, f, tri, ref, rec, cfg, ccfg, young, what, bins=None, fcfg=None, plain=None):
    """one fluxes -> column -> slab[_coupled] round as slab_ref.gpu_round / slab_fsd_ref.gpu_round run it (the designed flux and column rows through the
    device_rows doors), with the received rows `rec` put first; the column inside resets sst / sss to them, and so does the restatement"""
    clock = SR.clock()
    fe.ocean_coupled_put_rows(**{k: rec[k] for k in THREE})
    if bins is None:
        got, st, words, before, after = SR.gpu_round(fe, f, ref, DT, clock)
    else:
        got, st, words, words2, b1, b2, before, after = SFR.gpu_round(fe, f, ref, bins, DT, clock, True)
    ref["sst"], ref["sss"] = rec["ocean_temp"].copy(), rec["ocean_salt"].copy()                 # FE.cpp:5355-5356
    if plain is not None:
        un = SR.copy(ref)
        SR.slab(un, cfg, ccfg, ALB, tri, young, DT, clock)
        plain.update(un)
    if bins is None:
        rows, ref_words = OC.slab(ref, cfg, ccfg, ALB, tri, young, DT, clock)
    else:
        rows, ref_words, ref_words2, _ = OC.slab_coupled(ref, bins, cfg, ccfg, fcfg, ALB, tri, young, DT, clock)
        assert np.array_equal(words2, ref_words2), (what, "fsd branches")
    assert np.array_equal(words, ref_words), (what, "branches", np.flatnonzero(words != ref_words)[:5])
    for i, k in enumerate(SR.ROWS + SR.IN_PLACE):
        dev, want = (got[k], rows[k]) if i < len(SR.ROWS) else (st[k], ref[k])
        bad = np.flatnonzero(~SR.same_bits(dev, want))
        assert bad.size == 0, (what, k, bad.size, bad[:5], dev[bad[:3]], want[bad[:3]])
    assert _same(st["sst"], rec["ocean_temp"]) and _same(st["sss"], rec["ocean_salt"])           # not advanced by the call
    if bins is not None:
        assert _same(b1["conc_fsd"], bins["conc_fsd"]) and _same(b1["conc_mech_fsd"], bins["conc_mech_fsd"]), (what, "bins")
        SFR.update_fsd(ref, bins, fcfg, young)
        assert _same(b2["conc_fsd"], bins["conc_fsd"]) and _same(b2["conc_mech_fsd"], bins["conc_mech_fsd"]), (what, "bins after updateFSD")
        bins["conc_fsd"], bins["conc_mech_fsd"] = b2["conc_fsd"].copy(), b2["conc_mech_fsd"].copy()
    for k in SR.IN_PLACE:
        ref[k] = st[k].copy()
    return got, st


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
def test_slab_keeps_sst_and_sss_and_heals_from_the_received_salinity(thermo, young):
    p, lm, f, tri, inp, finp, strata, calm = TS._case("toy", young)
    inp = SR.copy(inp)
    ccfg = CR.default_config(thermo_type=thermo, freezingpoint_type="unesco")
    cfg = SR.category_config(young, temp_dep_healing=1)
    fe, f = SR.gpu_handle(p, lm, f, inp, finp, ccfg, cfg)
    fe.ocean_coupled_attach(None, rows=THREE)
    ref, plain = SR.copy(inp), {}
    for call in range(3):
        rec = OC.received_rows(ref, seed=40 + call)
        got, st = _slab_round(fe, f, tri, ref, rec, cfg, ccfg, young, f"{thermo} young={young} round {call}", plain=plain if call == 0 else None)
        if call == 0:                                                          # the Tbot path is live: the slab-ocean loop heals from the advanced salinity
            assert (st["time_relaxation_damage"] != plain["time_relaxation_damage"]).any()
            assert not _same(plain["sss"], rec["ocean_salt"]) and np.abs(got["delS"]).max() > 0
    fe.close()


@pytest.mark.parametrize("nb", [2, 7])
def test_slab_coupled_with_bins_takes_the_same_guards(nb):
    p, lm, f, tri, inp, fsd, finp = TSF._case("toy", True, nb)
    inp = SR.copy(inp)
    ccfg = CR.default_config(freezingpoint_type="unesco")
    cfg = SR.category_config(True, temp_dep_healing=1)
    fcfg = SFR.fsd_config(nb, True)
    fe, f = SR.gpu_handle(p, lm, f, inp, finp, ccfg, cfg)
    SFR.attach(fe, fsd, fcfg, True)
    fe.ocean_coupled_attach(None, rows=THREE)
    ref, bins = SR.copy(inp), SFR.copy_fsd(fsd, True)
    for call in range(2):
        rec = OC.received_rows(ref, seed=50 + call)
        _slab_round(fe, f, tri, ref, rec, cfg, ccfg, True, f"{nb} bins round {call}", bins=bins, fcfg=fcfg)
    fe.close()


# ---- end to end: the toy mesh's own map ---------------------------------------------------------------------------------------------------------------------

def _toy_fields(gx, gy):
    sx, sy = (gx - gx.mean()) / 5e4, (gy - gy.mean()) / 5e4
    return {"ocean_temp": -1.2 + 0.4 * np.sin(2. * sx) * np.cos(sy), "ocean_salt": 31. + 2. * np.cos(sx + sy), "qsrml": 0.5 + 0.4 * np.sin(3. * sx + sy),
            "wlbk": 30. + 25. * np.cos(2. * sy)}


def test_receive_then_fluxes_column_slab_on_the_toy_mesh():
    p, lm, f, tri, inp, finp, strata, calm = TS._case("toy", True)
    assert lm.num_elements == 2368
    inp = SR.copy(inp)
    ccfg = CR.default_config(freezingpoint_type="unesco")
    cfg = SR.category_config(True, temp_dep_healing=1)
    fe, f = SR.gpu_handle(p, lm, f, inp, finp, ccfg, cfg)
    gx, gy, cx, cy = TG._toy_grid(lm)
    rg, gmap = TG._make(lm.coord_x, lm.coord_y, np.ascontiguousarray(tri, np.int32), gx, gy, cx, cy)
    names = THREE + ("wlbk",)
    a, b, factor, bias = [1., 1., 1., 2.], [0., 0., 0., 0.], [1., 1., 1., 1.], [0., 0.5, 0., 0.]
    fe.ocean_coupled_attach(gmap, rows=names, a=a, b=b, factor=factor, bias=bias)
    fields = _toy_fields(gx, gy)
    dev = [TG.Dev((gx.size,), fields[k]) for k in names]
    fe.ocean_coupled_receive([d.p.value for d in dev], device=True)
    got = fe.ocean_coupled_get(names)
    want = dict(zip(names, OC.receive(gmap.export(), [fields[k] for k in names], a, b, factor, bias)))
    for k in names:
        assert _same(got[k], want[k]), k
    nan = np.isnan(got["ocean_temp"])
    assert 0 < nan.sum() < lm.num_elements // 4                                # boundary triangles no wet cell touches; far from "NaN everywhere"
    fe.ocean_coupled_receive([fields[k] for k in names])                       # host fields: the same rows
    again = fe.ocean_coupled_get(names)
    for k in names:
        assert _same(again[k], want[k]), k
    # fluxes: Qow from the device's own rows
    fe.fluxes()
    fl = fe.fluxes_get()
    assert _same(fl["Qow"], OC.qow(fl, want["qsrml"]))
    # column: the restatement on the device's flux rows
    young = True
    cin = dict(SR.copy(inp), tair=finp["tair"].copy(), tsurf_young=finp["tsurf_young"].copy(), snowfr=np.ones(lm.num_elements), ocean_temp=want["ocean_temp"],
               ocean_salt=want["ocean_salt"])
    for k in CR.FLUX_IN:
        cin[k], cin[k + "_young"] = fl[k], fl[k + "_young"]
    fe.column(DT)
    col = fe.column_rows()
    rows, _ = OC.column(cin, ccfg, tri, young, DT)
    for k in CR.ROWS:
        bad = np.flatnonzero(~SR.same_bits(col[k], rows[k]))
        assert bad.size == 0, ("column", k, bad[:5])
    st = fe.flux_get(("sst", "sss"))
    assert _same(st["sst"], want["ocean_temp"]) and _same(st["sss"], want["ocean_salt"])
    # slab: the restatement on the device's flux and column rows
    ref = SR.copy(inp)
    ref.update({"F:" + k: fl[k] for k in _abi.FLUX_ROWS})
    ref.update({"K:" + k: col[k] for k in _abi.COL_ROWS})
    for k in ("tice0", "tice1", "tice2", "h_young", "hs_young", "sst", "sss"):
        ref[k] = cin[k].copy()
    clock = SR.clock()
    fe.slab(DT, clock)
    srows = fe.slab_rows()
    words = fe.debug_array("slab_branches").astype(np.uint32)
    rrows, rwords = OC.slab(ref, cfg, ccfg, ALB, tri, young, DT, clock)
    dst = SR.device_state(fe)
    assert np.array_equal(words, rwords), np.flatnonzero(words != rwords)[:5]
    for i, k in enumerate(SR.ROWS + SR.IN_PLACE):
        dv, wt = (srows[k], rrows[k]) if i < len(SR.ROWS) else (dst[k], ref[k])
        bad = np.flatnonzero(~SR.same_bits(dv, wt))
        assert bad.size == 0, ("slab", k, bad.size, bad[:5], dv[bad[:3]], wt[bad[:3]])
    assert np.isfinite(srows["Qo"]).sum() > lm.num_elements // 2
    for d in dev:
        d.free()
    fe.close(); gmap.close(); rg.close()


def test_the_received_wlbk_row_feeds_the_breakup_from_the_device():
    n = 6
    cfg = FS.default_config(n, FS.standard_tables(n), True)
    Ne = TF._num_elements("toy")
    st, wlbk, g = FS.breakup_inputs(n, Ne, True, cfg["tables"])
    fe, twin = TF._handle("toy", True, st, cfg), TF._handle("toy", True, st, cfg)
    lm = fe.lm
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3) - 1, np.int32)
    gx, gy, cx, cy = TG._toy_grid(lm)
    rg, gmap = TG._make(lm.coord_x, lm.coord_y, tri, gx, gy, cx, cy)
    fe.ocean_coupled_attach(gmap, rows=("wlbk",), a=2.)                        # I_wlbk: a = 2, b = 0
    field = _toy_fields(gx, gy)["wlbk"]
    d = TG.Dev((gx.size,), field)
    fe.ocean_coupled_receive([d.p.value], device=True)
    rows, ptr = fe.ocean_coupled_get(("wlbk",), want_device=True)
    assert _same(rows["wlbk"], OC.receive(gmap.export(), [field], 2., 0., 1., 0.)[0]) and ptr["wlbk"] and not ptr["qsrml"]
    assert _refused(lambda: fe.ocean_coupled_get(("qsrml",)), STATE, "qsrml")
    fa = fe.fsd_breakup(ptr["wlbk"])
    fb = twin.fsd_breakup(rows["wlbk"])
    assert fa == fb
    ba, bb = fe.get_coupled(True, n), twin.get_coupled(True, n)
    assert _same(ba["conc_fsd"], bb["conc_fsd"]) and _same(ba["cum_damage"], bb["cum_damage"])
    assert not _same(ba["conc_fsd"], st["conc_fsd"])                           # (something broke)
    d.free(); fe.close(); twin.close(); gmap.close(); rg.close()


# ---- life cycle and refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_life_cycle_and_refusals():
    cfg = CR.default_config(freezingpoint_type="unesco")
    fe, p, lm, f, tri, inp, calm = TC._handle("toy", True, cfg)
    rec = OC.received_rows(inp)
    fe.diffusion_configure(1e2, 1e2, 1e4, 900.)
    fe.fluxes(); fe.column(DT)
    base = fe.column_rows()
    fe.flux_put(sst=inp["sst"], sss=inp["sss"], tice0=inp["tice0"], tsurf_young=inp["tsurf_young"])
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    fe.put_state(dict(f, h_young=inp["h_young"], hs_young=inp["hs_young"]))
    # not attached
    assert _refused(lambda: fe.ocean_coupled_put_rows(qsrml=rec["qsrml"]), STATE, "attach")
    assert _refused(lambda: fe.ocean_coupled_get(), STATE)
    # a map of the wrong size
    c, rg, other = TG._case_map("one_cell")
    assert _refused(lambda: fe.ocean_coupled_attach(other), INVALID, str(c["tri"].shape[0]), str(lm.num_elements))
    # attached, rows missing: each call names the row
    fe.ocean_coupled_attach(None, rows=THREE)
    assert _refused(fe.fluxes, STATE, "qsrml")
    fe.ocean_coupled_put_rows(qsrml=rec["qsrml"])
    fe.fluxes()
    assert _refused(lambda: fe.ocean_coupled_put_rows(wlbk=rec["wlbk"]), INVALID, "wlbk")
    assert _refused(lambda: fe.ocean_coupled_receive([rec["qsrml"]] * 3), STATE, "map")
    fe.ocean_coupled_put_rows(ocean_temp=rec["ocean_temp"], ocean_salt=rec["ocean_salt"])
    assert _refused(fe.diffuse, STATE, "FE.cpp:3934")
    # LINEAR freezing point
    fe.column_configure(**CR.default_config())
    assert _refused(lambda: fe.column(DT), STATE, "UNESCO", "FE.cpp:1246")
    fe.column_configure(**cfg)
    fe.column(DT)
    assert not _same(fe.column_rows(("Qio",))["Qio"], base["Qio"])
    # detach: the un-attached bits, and diffuse works again
    fe.ocean_coupled_detach()
    fe.flux_put(sst=inp["sst"], sss=inp["sss"], tice0=inp["tice0"], tsurf_young=inp["tsurf_young"])
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    fe.put_state(dict(f, h_young=inp["h_young"], hs_young=inp["hs_young"]))
    fe.fluxes(); fe.column(DT)
    again = fe.column_rows()
    for k in CR.ROWS:
        assert _same(again[k], base[k]), k
    fe.diffuse()
    # set_mesh drops the attachment and the rows
    fe.ocean_coupled_attach(None, rows=THREE)
    fe.ocean_coupled_put_rows(**{k: rec[k] for k in THREE})
    fe.set_mesh(lm)
    assert _refused(lambda: fe.ocean_coupled_get(), STATE)
    fe.ocean_coupled_attach(None, rows=THREE)
    assert _refused(lambda: fe.ocean_coupled_get(("qsrml",)), STATE, "qsrml")
    other.close(); rg.close(); fe.close()


def test_regrid_drops_the_attachment_and_the_rows():
    import cases
    from nextsim_amd import dynamics
    from test_gpu_regrid_handle import _fields, _global_mesh
    x, y, tri, ng = cases.rect_mesh(24, 1)
    p, lm, f = _fields(_global_mesh(x, y, tri, ng), True)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    Ne = lm.num_elements
    fe.ocean_coupled_attach(None, rows=THREE)
    fe.ocean_coupled_put_rows(ocean_temp=np.full(Ne, -1.), ocean_salt=np.full(Ne, 30.), qsrml=np.full(Ne, 0.5))
    assert _same(fe.ocean_coupled_get(("qsrml",))["qsrml"], np.full(Ne, 0.5))
    prev = np.arange(1, lm.num_nodes + 1, dtype=np.float64)                    # the same mesh again: every vertex survives
    info = fe.regrid(lm, prev, ng, {k: f[k] for k in dynamics.REGRID_INPUTS}, (), moved=(x, y))
    assert info["num_failed"] == 0
    assert _refused(lambda: fe.ocean_coupled_get(), STATE, "attached")
    assert _refused(lambda: fe.ocean_coupled_put_rows(qsrml=np.full(Ne, 0.5)), STATE, "attach")
    fe.ocean_coupled_attach(None, rows=THREE)
    assert _refused(lambda: fe.ocean_coupled_get(("qsrml",)), STATE, "qsrml")  # the row went with the old mesh
    fe.close()


def test_attach_receive_detach_cycles_return_the_device_memory():
    p, lm, f, tri, inp, finp, strata, calm = TS._case("toy", True)
    from nextsim_amd import dynamics
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    gx, gy, cx, cy = TG._toy_grid(lm)
    rg, gmap = TG._make(lm.coord_x, lm.coord_y, np.ascontiguousarray(tri, np.int32), gx, gy, cx, cy)
    L = TG._hip()
    fields = _toy_fields(gx, gy)
    names = ("ocean_temp", "ocean_salt", "qsrml", "mld", "wlbk")
    fields["mld"] = np.full(gx.size, 20.)

    def free_bytes():
        a, b = C.c_size_t(), C.c_size_t()
        assert L.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
        return a.value

    def cycle():
        fe.ocean_coupled_attach(gmap, rows=names)
        fe.ocean_coupled_receive([fields[k] for k in names])
        fe.ocean_coupled_get(names)
        fe.ocean_coupled_detach()
    cycle(); cycle()
    start = free_bytes()
    for _ in range(20):
        cycle()
    end = free_bytes()
    print(f"free device memory: {start} before, {end} after 20 cycles")
    assert end >= start
    fe.close(); gmap.close(); rg.close()
