"""tests/column_ref.py, the restatement of thermo()'s ice columns (FE.cpp:5306-5411) that the library is compared with: its designed inputs reach every branch
(the census), no element sits on an edge of a branch (so a comparison within a tolerance cannot flip one), two hand-computed columns, and the smallest terms are
each visible far above every tolerance tests/test_gpu_column.py uses.  No device, no library."""
import functools

import numpy as np
import pytest

import cases
import column_ref as R

CAP = 1e-9          # the cap of every bound of tests/test_gpu_column.py


@functools.lru_cache(maxsize=None)
def _case(kind):
    gm = cases.global_mesh(kind)
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, strata, calm = R.make_inputs(gm.x, gm.y, tri)
    return tri, inp, strata, calm


@functools.lru_cache(maxsize=None)
def _run(kind, thermo, qio="basic", snowfall_source="precip_snowfr"):
    tri, inp, strata, calm = _case(kind)
    cfg = R.default_config(thermo_type=thermo, qio_type=qio, snowfall_source=snowfall_source)
    return R.column(R.copy(inp), cfg, tri, True, R.DT)


@pytest.mark.parametrize("kind", ["small", "toy"])
def test_the_census(kind):
    tri, inp, strata, calm = _case(kind)
    Ne = tri.shape[0]
    least = max(8, int(np.ceil(0.02 * Ne)))

    def need(what, mask):
        assert np.count_nonzero(mask) >= least, (kind, what, int(np.count_nonzero(mask)), least)

    _, w = _run(kind, "winton")
    _, z = _run(kind, "zero_layer")
    for name, rec, sfx in (("old ice, WINTON", w, ""), ("old ice, ZERO_LAYER", z, ""), ("young ice", w, "_young")):
        need(name + ": conc <= 0", rec["noice" + sfx] == 1)
        need(name + ": voli <= 0 with conc > 0", rec["noice" + sfx] == 2)
    thick_w = (w["noice"] == 0) & (w["hmin"] == 0)
    need("thick ice with snow", thick_w & (inp["snow_thick"] > 0))
    need("thick ice without snow", thick_w & (inp["snow_thick"] == 0))
    for name, rec, sfx in (("old ice", z, ""), ("young ice", z, "_young")):     # thermoIce0
        g = lambda k: rec[k + sfx]
        need(name + ": Tsurf clamped at 0", (g("clamped") == 1) & (g("hs_pos") == 1))
        need(name + ": Tsurf clamped at Tfr_ice", (g("clamped") == 1) & (g("hs_pos") == 0))
        need(name + ": Tsurf not clamped", g("clamped") == 0)
        need(name + ": the snow melt exhausts the snow", g("snow_exhausted") == 1)
        need(name + ": snow left", g("snow_exhausted") == 0)
        need(name + ": flooding", g("flood") == 1)
        need(name + ": no flooding", g("flood") == 0)
        need(name + ": hi < hmin, del_hi < 0", (g("hmin") == 1) & (g("del_hi_neg") == 1))
        need(name + ": hi < hmin, del_hi >= 0", (g("hmin") == 1) & (g("del_hi_neg") == 0))
        need(name + ": hi >= hmin", g("hmin") == 0)
    need("Winton: Tsurf > Tfr_surf", w["surf_melt"] == 1)
    need("Winton: no surface melt", w["surf_melt"] == 0)
    for b in range(4):
        need(f"Winton: sublimation branch {b + 1}", w["subl_branch"] == b)
    need("Winton: Mbot <= 0", w["Mbot_pos"] == 0)
    need("Winton: Mbot > 0", w["Mbot_pos"] == 1)
    need("Winton: everything melts, bottom block", w["all_melts_bot"] == 1)
    need("Winton: not everything melts, bottom block", w["all_melts_bot"] == 0)
    need("Winton: everything melts, surface block", w["all_melts_surf"] == 1)
    need("Winton: flooding", w["flood"] == 1)
    need("Winton: h2 > h1", w["h2_gt_h1"] == 1)
    need("Winton: h2 <= h1", w["h2_gt_h1"] == 0)
    need("Winton: T2 > Tfr_ice", w["T2_warm"] == 1)
    need("Winton: T2 <= Tfr_ice", w["T2_warm"] == 0)
    need("Winton: hi < hmin", w["hmin"] == 1)
    _, t = _run(kind, "winton", snowfall_source="precip_tair")
    need("snowfall: tair < 0", t["snow_tair_neg"] == 1)
    need("snowfall: tair >= 0", t["snow_tair_neg"] == 0)
    assert calm.size >= 8
    Nn = inp["VT"].size // 2
    for j in range(3):
        n = tri[calm, j]
        assert np.array_equal(inp["VT"][n], inp["ocean"][n]) and np.array_equal(inp["VT"][n + Nn], inp["ocean"][n + Nn])
    q = R.ice_ocean_heatflux(inp, R.default_config(qio_type="exchange"), tri, 9., R.DT)
    other = np.setdiff1d(np.arange(Ne), calm)
    assert not q[calm].any() and np.count_nonzero(q[other]) > 0.8 * other.size    # (the norm is exactly 0 there; elsewhere Qio is 0 only in the two strata with sst == Tbot)


@pytest.mark.parametrize("qio", ["basic", "exchange"])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("kind", ["small", "toy"])
def test_no_element_sits_on_an_edge(kind, thermo, qio):
    """the branch record is unchanged when every input moves one unit in the last place either way and when Qio moves +-4 units: a device whose hypot differs
    from the host's in the last places takes the same branches"""
    tri, inp, strata, calm = _case(kind)
    cfg = R.default_config(thermo_type=thermo, qio_type=qio)
    _, rec = _run(kind, thermo, qio)
    for direction in (+1, -1):
        _, moved = R.column(R.moved_one_ulp(inp, direction), cfg, tri, True, R.DT)
        for k in rec:
            assert np.array_equal(rec[k], moved[k]), (k, direction, np.flatnonzero(rec[k] != moved[k])[:5])
    for shift in (+4, -4):
        _, moved = R.column(R.copy(inp), cfg, tri, True, R.DT, qio_shift=shift)
        for k in rec:
            assert np.array_equal(rec[k], moved[k]), (k, shift, np.flatnonzero(rec[k] != moved[k])[:5])


def _one(thermo, **rows):
    """one element; snow_cond = physical::ki so that the snow-equivalent thickness of the ice, M_ks*hi/ki, is hi"""
    tri = np.array([[0, 1, 2]])
    cfg = R.default_config(thermo_type=thermo, snow_cond=float(R.ki))
    z = np.zeros(1)
    inp = dict(VT=np.zeros(6), ocean=np.zeros(6), tair=z - 5., precip=z, snowfr=z, snowfall=z, ocean_temp=z, ocean_salt=z, mld=z + 9., sss=z + 32., sst=z - 0.055 * 32.,
               conc=z + 0.5, thick=z + 1., snow_thick=z, conc_young=z, h_young=z, hs_young=z, tsurf_young=z, tice0=z, tice1=z, tice2=z)
    for k in R.FLUX_IN:
        inp[k], inp[k + "_young"] = z.copy(), z.copy()
    inp.update({k: np.array([float(v)]) for k, v in rows.items()})
    inp = R.copy(inp)
    out, rec = R.column(inp, cfg, tri, False, R.DT)
    return {k: float(v[0]) for k, v in out.items()}, {k: float(inp[k][0]) for k in R.IN_PLACE}


def test_a_zero_layer_column_by_hand():
    """hi = 1 / 0.5 = 2 m of bare ice, Tbot = -0.055 * 32 = -1.76, Tsurf = -11.76: Qic = ki * 10 / 2 * 1.065 = 2.0334 * 5.325 = 10.827855 W/m^2.  With Qia equal to
    it the surface is in balance and stays; sst = Tbot, so Qio = 0; the ice grows at the bottom by Qic * dt / qi = 10.827855 * 900 / (333550 * 917)
    = 9745.0695 / 305865350 = 3.18607e-5 m."""
    out, st = _one("zero_layer", tice0=-11.76, Qia=10.827855)
    assert out["tfrw"] == pytest.approx(-1.76, abs=1e-15) and out["Qio"] == 0. and out["hi_old"] == 2.
    assert st["tice0"] == pytest.approx(-11.76, abs=1e-12)
    assert out["del_hi"] == pytest.approx(3.18607e-5, rel=1e-5) and out["hi"] == pytest.approx(2. + 3.18607e-5, abs=1e-9)
    assert out["hs"] == 0. and out["del_hs_mlt"] == 0. and out["mlt_hi_top"] == 0. and out["mlt_hi_bot"] == 0. and out["del_hi_s2i"] == 0.
    # and one that melts from below: sst = Tbot + 0.001 K gives Qio = 0.001 * 1025 * 4186.84 * 9 / 900 = 42.91511 W/m^2, del_hb = (10.827855 - 42.91511) * 900 / 305865350
    out, st = _one("zero_layer", tice0=-11.76, Qia=10.827855, sst=-1.759)
    assert out["Qio"] == pytest.approx(42.91511, rel=1e-6)
    assert out["del_hi"] == pytest.approx(-9.44158e-5, rel=1e-5) and out["mlt_hi_bot"] == out["del_hi"] and out["mlt_hi_top"] == 0.


def test_a_winton_column_in_steady_conduction_by_hand():
    """2 m of bare ice with the linear profile of a steady conductive flux ki * G, G = 5 K/m: Tbot = -1.76, T2 = Tbot - G hi/4 = -4.26, T1 = Tbot - 3 G hi/4 = -9.26,
    Tsurf = Tbot - G hi = -11.76, and Qia = ki * G = 10.167 W/m^2 at the surface.  Winton's (21), (6) and (15) then leave the three temperatures where they are;
    nothing melts; with Qio = 0 the bottom grows by (24): ki G dt / (qi - C rhoi (Tbot - Tfr_ice)) = 9150.3 / (305865350 + 1925700 * 1.485) = 9150.3 / 308725014.5
    = 2.9639e-5 m at Tbot, which (26) mixes into the lower layer: T2 = -4.26 + 2.9639e-5 * 2.5 / 1 = -4.259926."""
    out, st = _one("winton", tice0=-11.76, tice1=-9.26, tice2=-4.26, Qia=10.167, dQiadT=15.)
    assert st["tice0"] == pytest.approx(-11.76, abs=1e-9)
    assert out["del_hi"] == pytest.approx(2.9639e-5, rel=1e-4) and out["hi"] == pytest.approx(2. + 2.9639e-5, rel=1e-9) and out["hi_old"] == 2.
    assert st["tice2"] == pytest.approx(-4.259926, abs=1e-6)
    assert abs(st["tice1"] + 9.26) < 1e-3
    assert out["Qio"] == 0. and out["hs"] == 0. and out["del_hs_mlt"] == 0. and out["mlt_hi_top"] == 0. and out["mlt_hi_bot"] == 0. and out["del_hi_s2i"] == 0.


@pytest.mark.parametrize("term,thermo", [("gamma", "zero_layer"), ("one_minus_beta_I", "zero_layer"), ("B1_I", "winton"), ("E1_qi_Tfr_T1", "winton")])
def test_the_smallest_terms_are_visible(term, thermo):
    """each of the smallest terms, removed, moves some row by more than MARGIN: a thousand times the cap of the bounds of tests/test_gpu_column.py"""
    MARGIN = 1e3 * CAP
    tri, inp, strata, calm = _case("small")
    assert term in R.TERMS
    cfg = R.default_config(thermo_type=thermo)
    rows, _ = _run("small", thermo)
    work = R.copy(inp)
    less, _ = R.column(work, cfg, tri, True, R.DT, drop=(term,))
    moved = {}
    for k in R.ROWS:
        ok = np.isfinite(rows[k]) & np.isfinite(less[k])
        moved[k] = float(np.max(np.abs(less[k][ok] - rows[k][ok]) / np.maximum(1., np.abs(rows[k][ok]))))
    print(term, {k: f"{v:.2e}" for k, v in moved.items() if v})
    assert max(moved.values()) > MARGIN, (term, moved)
