"""tests/slab_ref.py, the restatement of FE.cpp:5413-6133 the slab kernel is compared with, checked on its own: hand-computed columns, the designed strata (each
holds its share of the toy mesh, every decision of the branch word is taken and not taken, no element sits on an edge), planted mistakes that some row must
notice, and the calendar helper nextsim_amd.dynamics.slab_clock.  No device."""
import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import slab_ref as R
from nextsim_amd import _abi, dynamics

ALB = FR.default_config()["ocean_albedo"]
MU = CR.default_config()["freezingpoint_mu"]
rhow, cpw, rhoi, rhos, Lf, ki, si = (float(v) for v in (R.rhow, R.cpw, R.rhoi, R.rhos, R.Lf, R.ki, R.si))
qi, qs = Lf * rhoi, Lf * rhos
TRI1 = np.array([[0, 1, 2]])
ALL = dict.fromkeys(_abi.SLAB_CLOCK, 1)
# every configuration the strata are designed for: (young, options, clock flags)
CONFIGS = [(True, {}, {}), (True, {}, ALL), (True, dict(melt_type=1), {}), (True, dict(use_meltponds=1, temp_dep_healing=1), {}), (True, dict(use_assim_flux=1), {}),
           (True, dict(reset_by_date=1), ALL), (False, dict(newice_type=1), {}), (False, dict(newice_type=2), ALL), (False, dict(newice_type=3), {}),
           (False, dict(newice_type=1, use_assim_flux=1, assim_flux_exponent=2.), {})]


@pytest.fixture(scope="module")
def case():
    gm = cases.global_mesh("toy")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, strata, calm = R.make_inputs(gm.x, gm.y, tri)
    return tri, inp, strata, calm


def run(inp, tri, young, opts=None, flags=None, thermo="winton", **kw):
    work = R.copy(inp)
    rows, words = R.slab(work, R.category_config(young, **(opts or {})), CR.default_config(thermo_type=thermo), ALB, tri, young, R.DT, R.clock(**(flags or {})), **kw)
    return rows, work, words


def one(young=False, opts=None, flags=None, thermo="zero_layer", **rows):
    inp = R.blank_inputs(1, 3, **rows)
    out, work, words = run(inp, TRI1, young, opts, flags, thermo)
    return {k: float(v[0]) for k, v in out.items()}, {k: float(v[0]) for k, v in work.items() if k != "wind"}, int(words[0])


def test_a_supercooled_ice_free_element_under_newice_type_1():
    sss, sst, Qow, mld = 30., -1.6499, 250., 9.
    tfrw = -MU * sss
    out, st, w = one(opts=dict(newice_type=1), sss=sss, sst=sst, **{"F:Qow": Qow, "K:tfrw": tfrw})
    tw_new = sst - R.DT * Qow / (mld * rhow * cpw)
    assert tw_new < tfrw and w & R.BIT["supercooled"]
    newice = (tfrw - tw_new) * mld * rhow * cpw / qi
    assert st["conc"] == pytest.approx(newice / 0.25, rel=1e-13) and st["thick"] == pytest.approx(newice, rel=1e-13)
    assert out["newice"] == pytest.approx(newice * 86400. / R.DT, rel=1e-13)
    # Qow is reset to what brings the water to the freezing point: the ocean ends there
    assert st["sst"] == pytest.approx(tfrw, abs=1e-13)
    assert st["age"] == R.DT and st["age_det"] == R.DT                  # new ice: w_age = 0, age = dt


def test_an_element_with_every_flux_zero_keeps_its_state_and_ages():
    rows = dict(conc=0.5, thick=1., snow_thick=0.1, sst=-1., sss=30., ridge_ratio=0.3, age=5e6, age_det=4e6, fyi_fraction=0.2, conc_myi=0.1, thick_myi=0.2, tice0=-5.,
                **{"K:tfrw": -MU * 30., "K:hi": 2., "K:hi_old": 2., "K:hs": 0.2})
    out, st, w = one(**rows, opts=dict(newice_type=1))
    for k in ("sst", "sss", "conc", "thick", "snow_thick", "ridge_ratio", "conc_myi", "thick_myi", "fyi_fraction", "tice0"):
        assert st[k] == rows[k], k
    assert st["age"] == 5e6 + R.DT and st["age_det"] == 4e6 + R.DT
    assert all(out[k] == 0. for k in R.ROWS if k not in ("albedo", "sialb")) and out["albedo"] == 0.5 * ALB
    assert w == R.BIT["conc_ge_cmin"]


def test_a_melt_out_element_hands_its_heat_to_the_ocean():
    conc, hi, hs, hi_old = 0.4, 0.005, 0.1, 0.02
    rows = dict(conc=conc, thick=conc * hi_old, snow_thick=conc * hs, sst=-1., sss=30., tice0=-5., tice1=-4., tice2=-3., age=5e6, age_det=5e6, fyi_fraction=0.3,
                conc_myi=0.2, thick_myi=0.003, freeze_days=2., ridge_ratio=0.2, **{"K:tfrw": -MU * 30., "K:hi": hi, "K:hi_old": hi_old, "K:hs": hs, "K:del_hi": hi - hi_old})
    out, st, w = one(**rows, opts=dict(newice_type=1), thermo="winton")
    assert w & R.BIT["limit"] and w & R.BIT["melt"] and w & R.BIT["no_ice_tracers"]
    Qow = out["Qa"] / (1. - conc)                                      # D_Qa = Qow * old_ow_fraction here (Qia = 0)
    assert Qow == pytest.approx(conc * (hi * qi + hs * qs) / R.DT, rel=1e-13)
    assert st["tice0"] == st["tice1"] == st["tice2"] == -MU * si
    assert all(st[k] == 0. for k in ("conc", "thick", "snow_thick", "ridge_ratio", "age", "age_det", "fyi_fraction", "conc_myi", "thick_myi", "freeze_days"))
    assert st["freeze_onset"] == 1.


def test_one_pond_element_by_hand():
    conc, hi, hs, Qia, tice0 = 0.5, 2., 0., -30., -4.
    pv0, lid0, top, precip = 0.08, 0.015, -0.002, 2e-5
    rows = dict(conc=conc, thick=conc * hi, sst=-1., sss=30., tice0=tice0, pond_volume=pv0, lid_volume=lid0, pond_fraction=0.25, precip=precip,
                **{"K:tfrw": -MU * 30., "K:hi": hi, "K:hi_old": hi, "K:mlt_hi_top": top, "F:Qia": Qia})
    out, st, w = one(**rows, opts=dict(newice_type=1, use_meltponds=1))
    avail = -top * rhoi / rhow + precip / rhow * R.DT
    pv = pv0 + 0.8 * avail * conc
    pf = np.sqrt(pv / 0.8)
    depth = min(0.8 * pf, 0.9 * hi)
    pv = depth * pf
    pf = min(pf, (lid0 + pv) / max(0.05, depth))
    lidth = max(1e-3, min(0.3, lid0 * rhow / rhoi / pf))
    Qic = (-MU * si - tice0) / lidth * ki
    dlid = max((min(Qia - Qic, 0.) + Qic) * R.DT / (rhoi * Lf) * rhoi / rhow * pf, -lid0)
    assert w & R.BIT["lid_exists"] and not w & (R.BIT["pond_flushed"] | R.BIT["lid_removed"] | R.BIT["lid_forms"])
    assert st["lid_volume"] == pytest.approx(lid0 + dlid, rel=1e-12) and st["pond_volume"] == pytest.approx(pv - dlid, rel=1e-12)
    assert st["pond_fraction"] == pytest.approx(pf, rel=1e-12)


def test_every_stratum_holds_its_share_and_every_decision_is_taken_on_both_sides(case):
    tri, inp, strata, calm = case
    Ne = tri.shape[0]
    counts = np.bincount(strata, minlength=len(R.STRATA))
    assert counts.min() >= 0.02 * Ne, dict(zip(R.STRATA, counts))
    seen, unseen = np.uint32(0), np.uint32(0)
    by = {}
    for young, opts, flags in CONFIGS:
        rows, work, words = run(inp, tri, young, opts, flags)
        seen |= np.bitwise_or.reduce(words)
        unseen |= np.bitwise_or.reduce(~words)
        by[(young, tuple(opts.items()), bool(flags))] = words
    for k in R.BRANCHES:
        assert seen & np.uint32(R.BIT[k]) and unseen & np.uint32(R.BIT[k]), k
    # the strata take the decisions they are built for
    S = {k: strata == i for i, k in enumerate(R.STRATA)}
    w = by[(True, (), False)]
    t = lambda name: R.took(w, name)
    assert t("supercooled")[S["sc_noice"] | S["sc_not_filled"] | S["sc_fills"] | S["thin_sc"]].all() and not t("supercooled")[S["plain"]].any()
    assert t("n4_not_filled")[S["sc_not_filled"]].all() and not t("n4_not_filled")[S["sc_fills"]].any() and t("n4_young")[S["sc_fills"]].all()
    assert t("n4_sharp")[S["sharp"]].all() and t("n4_no_room")[S["no_room"]].all() and not t("n4_no_room")[~S["no_room"]].any()
    assert t("melt")[S["melt_myi"]].all() and t("melt_side")[S["melt_myi"]].all() and t("melt")[S["melt_hi_zero"]].all() and not t("melt_side")[S["melt_hi_zero"]].any()
    assert t("limit")[S["melt_hi_zero"]].all() and not t("conc_ge_cmin")[S["melt_hi_zero"]].any()                  # out through conc < cmin
    assert t("limit")[S["meltout_hmin"]].all() and t("conc_ge_cmin")[S["meltout_hmin"]].all()                       # out through hi < hmin
    assert t("ridge")[S["plain"]].all() and t("del_c_neg")[S["melt_myi"]].all() and t("old_melt")[S["melt_myi"] | S["melt_nomyi"]].all()
    assert (inp["conc_myi"][S["melt_myi"]] > 0).all() and not inp["conc_myi"][S["melt_nomyi"]].any()
    assert t("sss_below_si")[S["sss_low"]].all() and t("denom_clamp")[S["denom_clamp"]].all() and not t("denom_clamp")[~S["denom_clamp"]].any()
    assert t("reset")[S["fd_at_onset0"]].all() and t("freeze_days_ge")[S["fd_at_onset1"]].all() and not t("reset")[S["fd_at_onset1"] | S["fd_below"]].any()
    assert not t("freeze_days_ge")[S["fd_below"]].any()
    w = by[(True, (("melt_type", 1),), False)]
    assert R.took(w, "melt")[S["no_room"]].all() and not R.took(w, "melt_side")[S["no_room"]].any() and (inp["conc"][S["no_room"]] == 1.).all()
    w = by[(True, (("use_meltponds", 1), ("temp_dep_healing", 1)), False)]
    t = lambda name: R.took(w, name)
    assert t("lid_exists")[S["pond_lid"]].all() and not t("lid_removed")[S["pond_lid"]].any() and t("lid_forms")[S["pond_lid_forms"]].all()
    assert not t("lid_removed")[S["pond_lid_forms"]].any() and t("lid_removed")[S["pond_thick_lid"] | S["pond_frozen"]].all() and t("lid_forms")[S["pond_frozen"]].all()
    assert t("pond_flushed")[S["thin_sc"] | S["sc_noice"]].all() and not t("heal_ice")[S["melt_hi_zero"]].any() and t("heal_ice")[S["plain"]].all()
    w = by[(True, (("use_assim_flux", 1),), False)]
    assert R.took(w, "assim")[S["assim_neg"]].all() and (inp["conc_upd"][S["assim_neg"]] < 0).all()
    w = by[(False, (("newice_type", 2),), True)]
    assert R.took(w, "n2_newice")[S["sc_noice"]].all() and R.took(w, "n2_hi_old")[S["plain"]].all()
    w = by[(False, (("newice_type", 3),), False)]
    assert R.took(w, "n3_h0")[S["thin_sc"]].all() and not R.took(w, "n3_h0")[S["plain"]].any()
    assert calm.size >= 12 and not FR.wind_speed_element(inp["wind"], tri)[calm].any()


@pytest.mark.parametrize("young,opts,flags", CONFIGS, ids=lambda v: str(v))
def test_no_element_sits_on_an_edge(case, young, opts, flags):
    """the branch word survives every input moved one unit in the last place either way, and Qassm and the wind speed moved by +-4 units: what lets the device
    test demand equal branches where the device's pow / hypot enter"""
    tri, inp, strata, calm = case
    cfg = R.category_config(young, **opts)
    _, _, words = run(inp, tri, young, opts, flags)
    base = R.edge_of_the_reference(inp, cfg, words)
    for direction in (+1, -1):
        moved = R.moved_one_ulp(inp, direction)
        _, _, w = run(moved, tri, young, opts, flags)
        bad = np.flatnonzero(R.edge_of_the_reference(inp, cfg, w) != base)
        assert bad.size == 0, (direction, bad[:5], [R.STRATA[i] for i in strata[bad[:5]]], [hex(int(v)) for v in (w[bad[:5]] ^ words[bad[:5]])])
    for shift in (+4, -4):
        kw = dict(qassm_shift=shift) if opts.get("use_assim_flux") else dict(wspeed_shift=shift) if opts.get("newice_type") == 3 else None
        if kw:
            _, _, w = run(inp, tri, young, opts, flags, **kw)
            assert np.array_equal(w, words), (kw, np.flatnonzero(w != words)[:5])


def _noticed(a, b):
    """the column's measure: the largest |a - b| / max(1, |b|) over every row, every row written in place and the branch word; NaN against a number counts"""
    worst = 0.
    with np.errstate(all="ignore"):
        for x, y in zip(a, b):
            x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
            both = np.isnan(x) & np.isnan(y)
            d = np.where(both | (x == y), 0., np.abs(x - y) / np.maximum(1., np.abs(y)))
            worst = max(worst, float(np.nan_to_num(d, nan=np.inf).max()))
    return worst


def _all_rows(res):
    rows, work, words = res
    return [rows[k] for k in R.ROWS] + [work[k] for k in R.IN_PLACE] + [R.took(words, k).astype(np.float64) for k in R.BRANCHES]   # (a row of 0 / 1 per decision)


HAND = {
    # the water lands exactly on the freezing point: the outcome is continuous there (newice = 0, Qow is reset to the value it has), so only the branch word can notice
    "tw_le": (False, dict(newice_type=1), {}, dict(sss=30., sst=-MU * 30., **{"K:tfrw": -MU * 30.})),
    # thin ice, strong supercooling, little room: newice * PhiF / hi_old exceeds 1 - M_conc
    "no_del_c_bound": (False, dict(newice_type=2), {}, dict(conc=0.9, thick=0.045, sss=30., sst=-1.649, **{"K:tfrw": -MU * 30., "K:hi": 0.05, "K:hi_old": 0.05, "F:Qow": 5000.})),
}
DESIGNED = {"del_vi_no_young": (True, {}, {}), "qow_not_scaled": (True, {}, {}), "no_room_no_thick": (True, {}, {}), "hs_wrong_side": (True, {}, {}),
            "si_not_eff": (True, {}, {}), "ridge_on_melt": (True, {}, {}), "qio_mean_no_young": (True, {}, {}), "w_age_new_conc": (True, {}, {}),
            "c_myi_max_no_young": (True, dict(reset_by_date=1), dict(myi_reset_now=1)), "freeze_days_after_conc": (True, {}, dict(last_step_of_day=1))}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_a_planted_mistake_is_noticed(case, mistake):
    tri, inp, strata, calm = case
    if mistake in HAND:
        young, opts, flags, rows = HAND[mistake]
        inp, tri = R.blank_inputs(1, 3, **rows), TRI1
    else:
        young, opts, flags = DESIGNED[mistake]
    good = _all_rows(run(inp, tri, young, opts, flags))
    bad = _all_rows(run(inp, tri, young, opts, flags, drop=(mistake,)))
    assert _noticed(bad, good) > 1e-6, mistake
    assert _noticed(_all_rows(run(inp, tri, young, opts, flags)), good) == 0.


def test_the_mistakes_cover_the_list():
    assert set(HAND) | set(DESIGNED) == set(R.MISTAKES) and len(R.MISTAKES) == 12


# ---- the calendar: day numbers since 1900-01-01 (core/include/date.hpp); 2000-01-01 is day 36524 (100 years, 24 leap days: 1900 is none)
DAY_2000 = 36524
SEP15, AUG01, OCT01, MAR03 = DAY_2000 + 258, DAY_2000 + 213, DAY_2000 + 274, DAY_2000 + 62


def test_slab_clock():
    clk = dynamics.slab_clock
    none = dict.fromkeys(_abi.SLAB_CLOCK, 0)
    assert clk(MAR03, 900) == dict(none, first_step_of_day=1)                                    # midnight: step_in_day = 1
    assert clk(MAR03 + 1. / 96, 900) == none
    assert clk(MAR03 + 95. / 96, 900) == dict(none, last_step_of_day=1)                          # step 96 of 96
    assert clk(MAR03 + 47. / 48, 1800) == dict(none, last_step_of_day=1) and clk(MAR03 + 47. / 48, 900) == none
    assert clk(SEP15, 900) == dict(none, first_step_of_day=1, fyi_reset_now=1, myi_reset_now=1)  # 15 September, the default reset date
    assert clk(SEP15 + 0.5, 900) == none                                                         # ... at midnight only
    assert clk(SEP15 - 1, 900) == dict(none, first_step_of_day=1) == clk(SEP15 + 1, 900)
    assert clk(AUG01, 900) == dict(none, first_step_of_day=1, onset_reset_now=1) and clk(AUG01 + 0.25, 900) == none
    assert clk(OCT01, 900, reset_date="1001") == dict(none, first_step_of_day=1, myi_reset_now=1)   # a reset date of one's own
    assert clk(SEP15, 900, reset_date="1001") == dict(none, first_step_of_day=1, fyi_reset_now=1)
    assert clk(OCT01, 900) == dict(none, first_step_of_day=1)
    assert clk(DAY_2000 + 59, 900) == dict(none, first_step_of_day=1)                            # 29 February 2000
    assert clk(59, 900, reset_date="0301") == dict(none, first_step_of_day=1, myi_reset_now=1)   # 1900 has no 29 February: day 59 is 1 March
    assert clk(MAR03, 86400) == dict(none, first_step_of_day=1, last_step_of_day=1)              # one step a day is its first and its last
