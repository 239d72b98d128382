"""A line-faithful restatement of the rest of thermo()'s slab loop in model/finiteelement.cpp ("FE.cpp"), FE.cpp:5413-6133 as a default (non-OASIS) build compiles
it: the assimilation flux (5415-5425), section 6 (5434-5646: newice_type 1 .. 4, melt_type 1, 2), the freeze-days block (5649-5682), the new concentration and
thickness with Winton's (38), (39), (26) (5685-5711), the limit block (5714-5728), section 7, section 8 with meltPonds (5812-5846, 6538-6627), section 9
(5854-5881), the diagnostics (5903-5976) and the age and type tracers (5980-6132).  Scalar per element (numpy float64 scalars: one rounding per operation, 0 / 0
is NaN as in C), every statement in the reference's operand order, no contraction; std::max / std::min keep the reference's argument order (column_ref._max,
_min).  The library calls: sqrt (numpy's, correctly rounded), round (halves away from zero, exact), pow -- the C library's through ctypes, the one
fluxes_ref loads -- and hypot through fluxes_ref.wind_speed_element (numpy's, which calls the C library's; math.hypot is Python's own and differs).
tests/test_slab_host_kernel.py holds both routes to glibc's bits against the kernel's source compiled for the host.  Beside the 29 rows slab() returns one word
per element with a bit per decision the element took, in the order of nextsim_amd._abi.SLAB_BRANCHES (NXS_SLAB_BR_* of include/nxs_dyn.h).

PARITY WITH THE REFERENCE IS NOT PINNED: model/ cannot be compiled here (boost, MPI, netCDF), so no binary of the reference produced these numbers; the
restatement is what the library (nxs_dyn_slab) and the kernel's source compiled for the host are compared with, and tests/test_slab_ref.py checks it against
hand-computed answers.  Not restated, all of it #ifdef OASIS: melt_type 3, the FSD branches of the limit block, redistributeThermoFSD, the in-loop weldingRoach,
the mechanical FSD healing of 9.b, the OceanType::COUPLED guards.  Shared by tests/test_slab_ref.py, test_slab_host_kernel.py, test_slab_abi.py and
test_gpu_slab.py.

Inputs: a dict of rows -- the 25 rows of nxs_dyn_fluxes as "F:<name>" and the 22 of nxs_dyn_column as "K:<name>" (names of nextsim_amd._abi.FLUX_ROWS, COL_ROWS),
both read-only; wind [2 Nn]; precip, mld, conc_upd [Ne]; and the IN_PLACE rows [Ne], which slab() updates like the reference."""
from __future__ import annotations

import ctypes

import numpy as np

import column_ref as CR
import fluxes_ref as FR
from column_ref import F, _max, _min, rhow, cpw, rhoi, rhos, Lf, C, ki, si, hmin, days_in_sec
from nextsim_amd import _abi

cmin = F(float.fromhex(CR._PHYS["cmin"]["hex"]))
days_in_sec = F(days_in_sec)
CONSTANTS = _abi.SLAB_CONSTANTS
ROWS = _abi.SLAB_ROWS
BRANCHES = _abi.SLAB_BRANCHES
BIT = {k: 1 << i for i, k in enumerate(BRANCHES)}
FLUX = tuple("F:" + k for k in _abi.FLUX_ROWS)
COL = tuple("K:" + k for k in _abi.COL_ROWS)
STATE = ("conc", "thick", "snow_thick", "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi", "time_relaxation_damage")   # nxs_dyn_state
FLUX_STATE = ("sst", "sss", "pond_fraction", "lid_volume")                                                                                      # nxs_dyn_flux_state
TICE = ("tice0", "tice1", "tice2")
SLAB_STATE = tuple(k for k in _abi.SLAB_STATE if k != "conc_upd")
IN_PLACE = STATE + FLUX_STATE + TICE + SLAB_STATE
DT = 900
NO_CLOCK = dict.fromkeys(_abi.SLAB_CLOCK, 0)
# the planted mistakes of tests/test_slab_ref.py: slab(drop=...) makes one of them
MISTAKES = ("tw_le", "del_vi_no_young", "no_del_c_bound", "qow_not_scaled", "no_room_no_thick", "hs_wrong_side", "si_not_eff", "ridge_on_melt", "qio_mean_no_young",
            "w_age_new_conc", "c_myi_max_no_young", "freeze_days_after_conc")

_pow = FR._LIBM.pow
_pow.restype, _pow.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]


def default_config(**over):
    """the defaults of model/options.cpp:329-331, 397-403, 428-449, 543-548 (tests/golden/reference_constants.json), named after nxs_dyn_slab_config"""
    opt = CR._FIX["options"]
    v = lambda k: opt[k]["value"]
    c = {"newice_type": int(v("thermo.newice_type")), "melt_type": int(v("thermo.melt_type")), "use_assim_flux": int(v("thermo.use_assim_flux")),
         "temp_dep_healing": int(v("dynamics.use_temperature_dependent_healing")), "use_meltponds": int(v("thermo.use_meltponds")),
         "reset_by_date": int(v("age.reset_by_date")), "include_young_ice": int(v("age.include_young_ice")), "equal_melting": int(v("age.equal_melting")),
         "hnull": v("thermo.hnull"), "PhiF": v("thermo.PhiF"), "PhiM": v("thermo.PhiM"), "h_young_min": v("thermo.h_young_min"), "h_young_max": v("thermo.h_young_max"),
         "assim_flux_exponent": v("thermo.assim_flux_exponent"), "reset_freeze_days": v("age.reset_freeze_days"),
         "meltpond_runoff_fraction": v("thermo.meltpond_runoff_fraction"), "meltpond_depth_to_fraction": v("thermo.meltpond_depth_to_fraction"),
         "time_relaxation_damage": float(days_in_sec) * v("dynamics.time_relaxation_damage"), "deltaT_relaxation_damage": v("dynamics.deltaT_relaxation_damage")}
    for k, val in over.items():
        if k not in c:
            raise KeyError(k)
        c[k] = val
    return c


def category_config(young, **over):
    """default_config() for a handle of the young-ice (newice_type 4) or of the classic category (newice_type 1 unless `over` names another)"""
    return default_config(**dict({} if young else {"newice_type": 1}, **over))


def _shift(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, F(np.inf) if n > 0 else F(-np.inf))
    return F(x)


def _round(x):
    """std::round: halves away from zero"""
    return np.floor(x + F(0.5)) if x >= 0 else -np.floor(-x + F(0.5))


def melt_ponds(cfg, mu, br, dt, hi, hs, iceSurfaceMelt, snowMelt, Qia, rain, M_conc, M_thick, tice0, pond_volume, lid_volume, pond_fraction):
    """meltPonds, FE.cpp:6538-6627.  Returns (M_pond_volume, M_lid_volume, D_pond_fraction, the branch bits)"""
    roff, dep2frac = F(cfg["meltpond_runoff_fraction"]), F(cfg["meltpond_depth_to_fraction"])
    hIceMin = F(0.1)
    concMin = F(0.1)
    max_lid_thickness = F(0.3)
    min_lid_thickness = F(1e-3)
    ice_to_water = rhoi / rhow
    snow_to_water = rhos / rhow
    water_to_ice = rhow / rhoi
    availableWater = -iceSurfaceMelt * ice_to_water - snowMelt * snow_to_water + rain / rhow * dt
    pond_volume = pond_volume + (1 - roff) * availableWater * M_conc
    if pond_volume <= 0. or M_conc <= concMin or M_thick / M_conc <= hIceMin:
        return F(0.), F(0.), F(0.), br | BIT["pond_flushed"]
    pond_fraction = np.sqrt(pond_volume / dep2frac)
    pond_fraction = _min(pond_fraction, 1. - hs / (hs + 0.2))
    pond_depth = _min(dep2frac * pond_fraction, 0.9 * hi)
    pond_volume = pond_depth * pond_fraction
    pond_depth = _max(0.05, pond_depth)
    pond_fraction = _min(pond_fraction, (lid_volume + pond_volume) / pond_depth)
    delLidVolume = F(0.)
    if lid_volume > 0. and pond_fraction > 1e-11:
        br |= BIT["lid_exists"]
        TPond = -mu * si
        lidThickness = _max(min_lid_thickness, _min(max_lid_thickness, lid_volume * water_to_ice / pond_fraction))
        Qic = (TPond - tice0) / lidThickness * ki
        delLidThickness = (_min(Qia - Qic, 0.) + Qic) * dt / (rhoi * Lf)
        delLidVolume = delLidThickness * ice_to_water * pond_fraction
        delLidVolume = _max(delLidVolume, -lid_volume)
    elif Qia > 0.:
        br |= BIT["lid_forms"]
        delLidVolume = dt * Qia / (rhoi * Lf) * ice_to_water
    lid_volume = lid_volume + delLidVolume
    pond_volume = pond_volume - delLidVolume
    if pond_volume <= 0. or lid_volume * water_to_ice / pond_fraction >= max_lid_thickness:
        return F(0.), F(0.), F(0.), br | BIT["lid_removed"]
    return pond_volume, lid_volume, pond_fraction, br


def slab(inp, cfg, ccfg, ocean_albedo, tri, young, dt, clock, drop=(), qassm_shift=0, wspeed_shift=0):
    """thermo(), FE.cpp:5413-6133.  cfg: default_config(); ccfg: column_ref.default_config() (thermo_type, freezingpoint_type, freezingpoint_mu, snow_cond,
    mld_source, constant_mld); ocean_albedo: the fluxes'; clock: the five flags of nxs_dyn_slab_clock.  Returns (the 29 rows, the branch words [Ne] uint32); the
    IN_PLACE rows of inp are updated.  drop: one of MISTAKES.  qassm_shift / wspeed_shift move Qassm (where the pow is taken) / the wind speed by that many units
    in the last place."""
    Ne = tri.shape[0]
    ddt = F(dt)
    dtime_step = F(dt)
    qi = Lf * rhoi
    qs = Lf * rhos
    winton = ccfg["thermo_type"] == "winton"
    mu, M_ks = F(ccfg["freezingpoint_mu"]), F(ccfg["snow_cond"])
    newice_type, melt_type = int(cfg["newice_type"]), int(cfg["melt_type"])
    assert 1 <= newice_type <= 4 and 1 <= melt_type <= 2
    rh0 = F(1.) / F(cfg["hnull"])
    rPhiF = F(1.) / F(cfg["PhiF"])
    PhiF, PhiM = F(cfg["PhiF"]), F(cfg["PhiM"])
    h_young_min = F(cfg["h_young_min"])
    h_young_max_sharp = F(.5) * (h_young_min + F(cfg["h_young_max"]))          # FE.cpp:1198
    reset_by_date = bool(cfg["reset_by_date"])
    use_young_ice_in_myi_reset = bool(cfg["include_young_ice"]) and reset_by_date   # FE.cpp:5649-5650
    if "c_myi_max_no_young" in drop:
        use_young_myi_max = False
    else:
        use_young_myi_max = use_young_ice_in_myi_reset
    freeze_days_threshold = F(cfg["reset_freeze_days"])
    time_relaxation_damage, deltaT_relaxation_damage = F(cfg["time_relaxation_damage"]), F(cfg["deltaT_relaxation_damage"])
    M_ocean_albedo = F(ocean_albedo)
    out = {k: np.zeros(Ne) for k in ROWS}
    words = np.zeros(Ne, np.uint32)
    wspeed_row = None
    if newice_type == 3:
        wspeed_row = FR.wind_speed_element(inp["wind"], tri)
    fl = {k[2:]: inp[k] for k in FLUX}
    co = {k[2:]: inp[k] for k in COL}
    z = F(0.)
    with np.errstate(all="ignore"):
        for i in range(Ne):
            br = 0
            Qow = F(fl["Qow"][i])
            Qlw_ow, Qsw_ow, Qlh_ow, Qsh_ow, evap = fl["Qlw_ow"][i], fl["Qsw_ow"][i], fl["Qlh_ow"][i], fl["Qsh_ow"][i], fl["evap"][i]
            Qia, Qlwi, Qswi, Qlhi, Qshi, albedo = fl["Qia"][i], fl["Qlwi"][i], fl["Qswi"][i], fl["Qlhi"][i], fl["Qshi"][i], fl["albedo"][i]
            if young:
                Qia_young, Qlw_young, Qsw_young, Qlh_young, Qsh_young, albedo_young = (fl[k + "_young"][i] for k in ("Qia", "Qlw", "Qsw", "Qlh", "Qsh", "albedo"))
            else:
                Qia_young = Qlw_young = Qsw_young = Qlh_young = Qsh_young = albedo_young = z                   # FE.cpp:5265-5273
            tmp_snowfall, Qdw, Fdw, tfrw = co["snowfall"][i], co["Qdw"][i], co["Fdw"][i], co["tfrw"][i]
            Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i = (F(co[k][i]) for k in CR.ICE_ROWS)
            Qio_young, _, _, _, del_hi_young, del_hs_young_mlt, mlt_hi_top_young, mlt_hi_bot_young, del_hi_s2i_young = (F(co[k][i]) for k in CR.YOUNG_ROWS)
            M_precip = inp["precip"][i]
            mld = F(inp["mld"][i]) if ccfg["mld_source"] == "row" else F(ccfg["constant_mld"])
            M_conc, M_thick, M_ridge_ratio = F(inp["conc"][i]), F(inp["thick"][i]), F(inp["ridge_ratio"][i])
            M_conc_myi, M_thick_myi = F(inp["conc_myi"][i]), F(inp["thick_myi"][i])
            M_conc_young = M_h_young = M_hs_young = z
            if young:
                M_conc_young, M_h_young, M_hs_young = F(inp["conc_young"][i]), F(inp["h_young"][i]), F(inp["hs_young"][i])
            M_sst, M_sss = F(inp["sst"][i]), F(inp["sss"][i])
            tice0 = F(inp["tice0"][i])
            tice1, tice2 = (F(inp["tice1"][i]), F(inp["tice2"][i])) if winton else (z, z)
            M_del_vi_tend, M_freeze_days, M_freeze_onset = F(inp["del_vi_tend"][i]), F(inp["freeze_days"][i]), F(inp["freeze_onset"][i])
            M_conc_summer, M_thick_summer = F(inp["conc_summer"][i]), F(inp["thick_summer"][i])
            M_fyi_fraction, M_age_det, M_age = F(inp["fyi_fraction"][i]), F(inp["age_det"][i]), F(inp["age"][i])
            old_vol = M_thick
            old_conc = M_conc
            old_conc_young = M_conc_young
            old_conc_tot = old_conc + old_conc_young
            old_ow_fraction = 1. - old_conc_tot

            # FE.cpp:5413-5425
            Qassm = z
            if cfg["use_assim_flux"]:
                M_conc_upd = F(inp["conc_upd"][i])
                conc_pre_assim = old_conc + old_conc_young - M_conc_upd
                if conc_pre_assim > 0 and M_conc_upd < 0:
                    br |= BIT["assim"]
                    Qassm = (Qow * old_ow_fraction + Qio * old_conc + Qio_young * old_conc_young) * (
                        F(_pow(float(M_conc_upd / conc_pre_assim + 1), float(cfg["assim_flux_exponent"]))) - 1)
                    Qassm = _shift(Qassm, qassm_shift)

            # 6) FE.cpp:5434-5646
            tw_new = M_sst - ddt * (Qow + Qassm) / (mld * rhow * cpw)
            newice = z
            if (tw_new <= tfrw) if "tw_le" in drop else (tw_new < tfrw):
                br |= BIT["supercooled"]
                newice = old_ow_fraction * (tfrw - tw_new) * mld * rhow * cpw / qi
                Qow = -(tfrw - M_sst) * mld * rhow * cpw / ddt
            newice_stored = newice
            del_vi = newice + del_hi * old_conc
            mlt_vi_top = mlt_hi_top * old_conc
            mlt_vi_bot = mlt_hi_bot * old_conc
            del_vs_mlt = del_hs_mlt * old_conc
            snow2ice = del_hi_s2i * old_conc
            del_vi_young = z
            if young:
                del_vi_young = del_vi_young + del_hi_young * old_conc_young
                if "del_vi_no_young" not in drop:
                    del_vi = del_vi + del_hi_young * old_conc_young
                mlt_vi_top = mlt_vi_top + mlt_hi_top_young * old_conc_young
                mlt_vi_bot = mlt_vi_bot + mlt_hi_bot_young * old_conc_young
                snow2ice = snow2ice + del_hi_s2i_young * old_conc_young
                del_vs_mlt = del_vs_mlt + del_hs_young_mlt * old_conc_young
            del_c = z
            newsnow = z
            if newice_type == 1:
                del_c = newice * rh0
            elif newice_type == 2:
                if hi_old > 0.:
                    br |= BIT["n2_hi_old"]
                    del_c = newice * PhiF / hi_old
                elif newice > 0.:
                    br |= BIT["n2_newice"]
                    del_c = F(1.)
                else:
                    del_c = z
            elif newice_type == 3:
                wspeed = _shift(F(wspeed_row[i]), wspeed_shift)
                h0 = (1. + 0.1 * wspeed) / 15.
                if rPhiF * hi_old < h0:
                    br |= BIT["n3_h0"]
                del_c = newice / _max(rPhiF * hi_old, h0)
            else:
                M_h_young = M_h_young + newice
                M_conc_young = _min(1. - M_conc, M_conc_young + newice / h_young_min)
                newice = z
                newsnow = z
                if M_conc_young > 0.:
                    br |= BIT["n4_young"]
                    if M_h_young < h_young_min * M_conc_young:
                        br |= BIT["n4_not_filled"]
                        M_conc_young = M_h_young / h_young_min
                    else:
                        hiy = M_h_young / M_conc_young
                        if hiy > h_young_max_sharp:
                            br |= BIT["n4_sharp"]
                            hsy = _max(0., M_hs_young / M_conc_young)
                            tmp = M_conc_young * (h_young_max_sharp - h_young_min) / (hiy - h_young_min)
                            del_c = _max(0., M_conc_young - tmp)
                            M_conc_young = tmp
                            tmp = M_conc_young * h_young_max_sharp
                            newice = _max(0., M_h_young - tmp)
                            M_h_young = tmp
                            tmp = M_conc_young * hsy
                            newsnow = _max(0., M_hs_young - tmp)
                            M_hs_young = tmp
                else:
                    br |= BIT["n4_no_room"]
                    if "no_room_no_thick" not in drop:
                        M_thick = M_thick + M_h_young
                    newice = M_h_young
                    newsnow = M_hs_young
                    M_h_young = z
                    M_hs_young = z
            if "no_del_c_bound" not in drop:
                del_c = _min(1. - M_conc, del_c)
            if del_hi < 0.:
                br |= BIT["melt"]
                if melt_type == 1:
                    if M_conc < 1.:
                        br |= BIT["melt_side"]
                        del_c = del_c + del_hi * M_conc * PhiM / hi_old
                    else:
                        del_c = del_c + 0.
                else:
                    if hi > 0.:
                        br |= BIT["melt_side"]
                        del_c = del_c + PhiM * (1. - M_conc) * _min(0., Qow) * ddt / (hi * qi + hs * qs)
                        if "qow_not_scaled" not in drop:
                            Qow = Qow * (1. - PhiM)
                    else:
                        del_c = -M_conc

            def freeze_days_block(M_conc, M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br):   # FE.cpp:5649-5682
                if clock["first_step_of_day"]:
                    M_del_vi_tend = z
                M_del_vi_tend = M_del_vi_tend + del_vi * ddt
                if clock["last_step_of_day"]:
                    if M_del_vi_tend > 0.:
                        br |= BIT["day_freeze"]
                        M_freeze_days = M_freeze_days + 1.
                    elif M_del_vi_tend < 0.:
                        br |= BIT["day_melt"]
                        M_freeze_days = z
                        conc_summer = M_conc + _min(0., del_c)
                        thick_summer = M_thick + _min(0., del_vi)
                        if young and use_young_ice_in_myi_reset:
                            conc_summer = conc_summer + M_conc_young
                            thick_summer = thick_summer + M_h_young
                        M_conc_summer = _max(0., _min(1., conc_summer))
                        M_thick_summer = _max(0., thick_summer)
                return M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br

            if "freeze_days_after_conc" not in drop:
                M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br = freeze_days_block(M_conc, M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br)
            # FE.cpp:5685-5711
            M_conc = M_conc + del_c
            if "freeze_days_after_conc" in drop:
                M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br = freeze_days_block(M_conc, M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br)
            if M_conc >= cmin:
                br |= BIT["conc_ge_cmin"]
                hi = (hi * old_conc + newice) / M_conc
                if del_c < 0.:
                    br |= BIT["del_c_neg"]
                if (del_c >= 0.) if "hs_wrong_side" in drop else (del_c < 0.):
                    Qow = Qow - del_c * hs * qs / ddt
                else:
                    hs = (hs * old_conc + newsnow) / M_conc
                if winton:
                    f1 = M_thick / (M_thick + newice)
                    Tbar = f1 * (tice1 - Lf * mu * si / (C * tice1)) + (1 - f1) * tfrw
                    tice1 = (Tbar - np.sqrt(Tbar * Tbar + 4 * mu * si * Lf / C)) / 2.
                    tice2 = f1 * tice2 + (1 - f1) * tfrw
            # FE.cpp:5714-5728
            if M_conc < cmin or hi < hmin:
                br |= BIT["limit"]
                Qow = Qow + (M_conc * hi * qi / ddt + M_conc * hs * qs / ddt)
                M_conc = z
                tice0 = -mu * si
                if winton:
                    tice1 = tice2 = -mu * si
                hi = z
                hs = z
                M_ridge_ratio = z
            # 7)
            M_thick = hi * M_conc
            M_snow_thick = hs * M_conc
            # 8) FE.cpp:5812-5846
            rain_on_ice = _max(0., M_precip - tmp_snowfall)
            rain = (1. - old_conc - old_conc_young) * M_precip + (old_conc + old_conc_young) * rain_on_ice
            emp = evap * (1. - old_conc - old_conc_young) - rain
            if cfg["use_meltponds"]:
                pv, lv, pf, br = melt_ponds(cfg, mu, br, ddt, hi, hs, mlt_hi_top, del_hs_mlt, Qia, rain_on_ice, M_conc, M_thick, tice0, F(inp["pond_volume"][i]),
                                            F(inp["lid_volume"][i]), F(inp["pond_fraction"][i]))
                inp["pond_volume"][i], inp["lid_volume"][i], inp["pond_fraction"][i] = pv, lv, pf
            if "qio_mean_no_young" in drop:
                Qio_mean = Qio * old_conc
            else:
                Qio_mean = Qio * old_conc + Qio_young * old_conc_young
            Qow_mean = Qow * old_ow_fraction
            M_sst = M_sst - ddt * (Qio_mean + Qow_mean - Qdw + Qassm) / (rhow * cpw * mld)
            denominator = (mld * rhow - del_vi * rhoi - (del_vs_mlt * rhos + (emp - Fdw) * ddt))
            if not (denominator > 1. * rhow):
                br |= BIT["denom_clamp"]
                denominator = 1. * rhow
            si_eff = si if "si_not_eff" in drop else _min(M_sss, si)
            if M_sss < si:
                br |= BIT["sss_below_si"]
            delsss = ((M_sss - si_eff) * rhoi * del_vi + M_sss * (del_vs_mlt * rhos + (emp - Fdw) * ddt)) / denominator
            M_sss = M_sss + delsss
            if M_thick > old_vol:
                br |= BIT["ridge"]
            if (M_thick > old_vol) or ("ridge_on_melt" in drop and M_thick > 0.):
                M_ridge_ratio = M_ridge_ratio * (old_vol / M_thick)
            # 9) FE.cpp:5854-5881
            if cfg["temp_dep_healing"]:
                if M_thick > 0.:
                    br |= BIT["heal_ice"]
                    Tbot = F(CR.freezing_point(ccfg, M_sss))
                    if not winton:
                        Cc = ki * M_snow_thick / (M_ks * M_thick)
                        deltaT = _max(1e-36, Tbot - tice0) / (1. + Cc)
                    else:
                        Cc = ki * M_snow_thick / (M_ks * M_thick / 4.)
                        deltaT = _max(1e-36, Tbot + Cc * (Tbot - tice1) - tice0) / (1. + Cc)
                    inp["time_relaxation_damage"][i] = _max(time_relaxation_damage * deltaT_relaxation_damage / deltaT, ddt)
                else:
                    inp["time_relaxation_damage"][i] = 1e36
            # 10) FE.cpp:5903-5976
            o = {}
            o["Qa"] = Qia * old_conc + Qia_young * old_conc_young + Qow * old_ow_fraction
            o["Qsw"] = Qswi * old_conc + Qsw_young * old_conc_young + Qsw_ow * old_ow_fraction
            o["Qlw"] = Qlwi * old_conc + Qlw_young * old_conc_young + Qlw_ow * old_ow_fraction
            o["Qsh"] = Qshi * old_conc + Qsh_young * old_conc_young + Qsh_ow * old_ow_fraction
            o["Qlh"] = Qlhi * old_conc + Qlh_young * old_conc_young + Qlh_ow * old_ow_fraction
            o["Qo"] = Qio_mean + Qow_mean
            o["Qnosun"] = Qio_mean + old_ow_fraction * (Qlw_ow + Qlh_ow + Qsh_ow)
            o["Qsw_ocean"] = old_ow_fraction * Qsw_ow
            o["Qassim"] = Qassm
            o["delS"] = delsss * rhow * mld * days_in_sec / dtime_step
            o["fwflux_ice"] = -1. / ddt * ((1. - 1e-3 * si_eff) * rhoi * del_vi + rhos * del_vs_mlt)
            o["fwflux"] = o["fwflux_ice"] - emp
            o["brine"] = -1e-3 * si_eff * rhoi * del_vi / ddt
            o["evap"] = evap * (1. - old_conc - old_conc_young)
            o["rain"] = rain
            o["vice_melt"] = del_vi * days_in_sec / ddt
            o["del_vi_young"] = del_vi_young * days_in_sec / ddt
            o["del_hi"] = del_hi * days_in_sec / ddt
            o["del_hi_young"] = del_hi_young * days_in_sec / ddt
            o["newice"] = newice_stored * days_in_sec / ddt
            o["mlt_top"] = mlt_vi_top * days_in_sec / ddt
            o["mlt_bot"] = mlt_vi_bot * days_in_sec / ddt
            o["snow2ice"] = snow2ice * days_in_sec / ddt
            sialb = old_conc * albedo
            if young:
                sialb = sialb + old_conc_young * albedo_young
            o["albedo"] = sialb + _max(0., old_ow_fraction) * M_ocean_albedo
            o["sialb"] = (sialb / old_conc_tot) if old_conc_tot > 0. else z
            # 10) FE.cpp:5980-6132
            del_vi_rplnt_myi = del_ci_rplnt_myi = del_vi_mlt_myi = del_ci_mlt_myi = z
            if M_conc < cmin or M_thick < M_conc * hmin:
                br |= BIT["no_ice_tracers"]
                M_fyi_fraction = M_age_det = M_age = M_thick_myi = M_conc_myi = M_freeze_days = z
                M_freeze_onset = F(1.)
            else:
                if clock["fyi_reset_now"]:
                    M_fyi_fraction = z
                else:
                    conc_fyi = M_fyi_fraction + del_c
                    M_fyi_fraction = _max(0., _min(1., conc_fyi))
                if "w_age_new_conc" in drop:
                    w_age = z if M_conc <= 0 else _min(M_conc / M_conc, 1.)
                else:
                    w_age = z if old_conc <= 0 else _min(old_conc / M_conc, 1.)
                M_age_det = w_age * (M_age_det + ddt) + _max((1 - w_age) * ddt, 0.)
                w_age = z if old_vol <= 0 else _min(old_vol / M_thick, 1.)
                M_age = w_age * (M_age + ddt) + _max((1 - w_age) * ddt, 0.)
                reset_myi = False
                if reset_by_date:
                    if clock["myi_reset_now"]:
                        reset_myi = True
                elif M_freeze_days >= freeze_days_threshold:
                    br |= BIT["freeze_days_ge"]
                    if M_freeze_onset <= 0.5:
                        reset_myi = True
                        M_freeze_onset = F(1.)
                if clock["onset_reset_now"]:
                    M_freeze_onset = z
                    ctot = M_conc
                    if young:
                        ctot = ctot + M_conc_young
                    if ctot == 0.:
                        M_freeze_onset = F(1.)
                    conc_summer = M_conc
                    thick_summer = M_thick
                    if young and use_young_ice_in_myi_reset:
                        conc_summer = conc_summer + M_conc_young
                        thick_summer = thick_summer + M_h_young
                    M_conc_summer = _max(0., _min(1., conc_summer))
                    M_thick_summer = _max(0., thick_summer)
                M_freeze_onset = F(_round(M_freeze_onset))
                old_conc_myi = M_conc_myi
                old_thick_myi = M_thick_myi
                c_myi_max = M_conc
                v_myi_max = M_thick
                if young and use_young_myi_max:
                    c_myi_max = c_myi_max + M_conc_young
                    v_myi_max = v_myi_max + M_h_young
                if reset_myi:
                    br |= BIT["reset"]
                    if not reset_by_date:
                        c_myi_reset = _max(M_conc_summer, M_conc_myi)
                        v_myi_reset = _max(M_thick_summer, M_thick_myi)
                        M_conc_myi = _min(c_myi_max, c_myi_reset)
                        M_thick_myi = _min(v_myi_max, v_myi_reset)
                    else:
                        M_conc_myi = c_myi_max
                        M_thick_myi = v_myi_max
                    M_conc_myi = _max(0., _min(1., M_conc_myi))
                    M_thick_myi = _max(0., M_thick_myi)
                    del_ci_rplnt_myi = M_conc_myi - old_conc_myi
                    del_vi_rplnt_myi = M_thick_myi - old_thick_myi
                elif M_thick < old_vol and old_conc > 0 and old_vol > 0:
                    br |= BIT["old_melt"]
                    if cfg["equal_melting"]:
                        del_c_ratio = _min(M_conc / old_conc, 1.)
                        del_v_ratio = _min(M_thick / old_vol, 1.)
                        del_ci_mlt_myi = _min(0., M_conc_myi * (del_c_ratio - 1.))
                        del_vi_mlt_myi = _min(0., M_thick_myi * (del_v_ratio - 1.))
                    M_conc_myi = _max(0., _min(c_myi_max, M_conc_myi + del_ci_mlt_myi))
                    M_thick_myi = _max(0., _min(v_myi_max, M_thick_myi + del_vi_mlt_myi))
                    del_ci_mlt_myi = M_conc_myi - old_conc_myi
                    del_vi_mlt_myi = M_thick_myi - old_thick_myi
            o["del_ci_mlt_myi"] = del_ci_mlt_myi * days_in_sec / ddt
            o["del_vi_mlt_myi"] = del_vi_mlt_myi * days_in_sec / ddt
            o["del_ci_rplnt_myi"] = del_ci_rplnt_myi * days_in_sec / ddt
            o["del_vi_rplnt_myi"] = del_vi_rplnt_myi * days_in_sec / ddt
            for k in ROWS:
                out[k][i] = o[k]
            inp["conc"][i], inp["thick"][i], inp["snow_thick"][i], inp["ridge_ratio"][i] = M_conc, M_thick, M_snow_thick, M_ridge_ratio
            inp["conc_myi"][i], inp["thick_myi"][i] = M_conc_myi, M_thick_myi
            if young:
                inp["conc_young"][i], inp["h_young"][i], inp["hs_young"][i] = M_conc_young, M_h_young, M_hs_young
            inp["sst"][i], inp["sss"][i], inp["tice0"][i] = M_sst, M_sss, tice0
            if winton:
                inp["tice1"][i], inp["tice2"][i] = tice1, tice2
            inp["del_vi_tend"][i], inp["freeze_days"][i], inp["freeze_onset"][i] = M_del_vi_tend, M_freeze_days, M_freeze_onset
            inp["conc_summer"][i], inp["thick_summer"][i] = M_conc_summer, M_thick_summer
            inp["fyi_fraction"][i], inp["age_det"][i], inp["age"][i] = M_fyi_fraction, M_age_det, M_age
            words[i] = br
    return {k: np.ascontiguousarray(out[k], np.float64) for k in ROWS}, words


def took(words, name):
    return (words & np.uint32(BIT[name])) != 0


# ---- designed inputs: every element belongs to one stratum, and a stratum is built to take one decision (tests/test_slab_ref.py counts them)
STRATA = ("plain", "sc_noice", "sc_not_filled", "sc_fills", "sharp", "no_room", "melt_myi", "melt_nomyi", "melt_hi_zero", "meltout_hmin", "assim_neg", "sss_low",
          "denom_clamp", "pond_lid", "pond_lid_forms", "pond_thick_lid", "pond_frozen", "fd_at_onset0", "fd_at_onset1", "fd_below", "thin_sc")


def make_inputs(x, y, tri, seed=5):
    """Inputs on a mesh (node coordinates, [Ne, 3] 0-based triangles): DESIGNED STRATA, not noise; the flux and column rows are designed directly (they are what
    sections 2 to 5 hand on), consistent with the state where the loop relies on it (thick = conc * hi_old, hi = hi_old + del_hi or 0).  The freezing point is the
    linear one of the default freezingpoint_mu.  Returns (inp, strata [Ne], calm: the elements whose three nodes have no wind at all)."""
    rng = np.random.default_rng(seed)
    Nn, Ne = x.size, tri.shape[0]
    s = rng.permutation(Ne) % len(STRATA)
    S = {k: i for i, k in enumerate(STRATA)}
    is_ = lambda *names: np.isin(s, [S[k] for k in names])
    r = lambda a, b: a + (b - a) * rng.random(Ne)
    mu = CR.default_config()["freezingpoint_mu"]
    inp = {}
    wind = 16. * (rng.random(2 * Nn) - 0.5)
    calm = np.sort(rng.choice(Ne, 40, replace=False))
    for nd in np.unique(tri[calm]):
        wind[nd] = wind[nd + Nn] = 0.
    inp["wind"] = wind
    # the ocean
    sss = r(28., 35.)
    sss[is_("sss_low")] = r(2., 4.)[is_("sss_low")]
    tfrw = -mu * sss
    dsst = r(0.05, 0.3)
    Qow = r(20., 80.)
    sc = is_("sc_noice", "sc_not_filled", "sc_fills", "thin_sc")
    dsst[sc], Qow[sc] = r(1e-4, 3e-4)[sc], r(200., 400.)[sc]
    melt = is_("melt_myi", "melt_nomyi", "melt_hi_zero", "meltout_hmin", "no_room")
    Qow[melt] = r(-100., -50.)[melt]
    inp.update({"sss": sss, "sst": tfrw + dsst})
    # the old ice
    conc, hi_old, hs = r(0.3, 0.7), r(1., 3.), r(0.1, 0.3)
    del_hi = r(0.001, 0.003)
    del_hi[melt] = -r(0.002, 0.01)[melt]
    m = is_("thin_sc")
    hi_old[m] = r(0.04, 0.06)[m]
    m = is_("denom_clamp")
    del_hi[m], conc[m] = r(11., 13.)[m], r(0.9, 0.95)[m]
    conc[is_("no_room")] = 1.
    hi = hi_old + del_hi
    m = is_("meltout_hmin")
    hi_old[m] = r(0.02, 0.03)[m]
    hi[m] = r(0.004, 0.008)[m]
    del_hi[m] = (hi - hi_old)[m]
    m = is_("melt_hi_zero")
    hi[m], hs[m], del_hi[m] = 0., 0., -hi_old[m]
    m = is_("pond_lid", "pond_lid_forms", "pond_thick_lid", "pond_frozen")
    hs[m] = r(0., 0.02)[m]
    noice = is_("sc_noice")
    for a in (conc, hi_old, hi, hs, del_hi):
        a[noice] = 0.
    mlt_top = np.where(del_hi < 0, 0.3 * del_hi, 0.)
    mlt_bot = np.where(del_hi < 0, 0.7 * del_hi, 0.)
    del_hs_mlt = np.where(noice | is_("pond_frozen"), 0., -r(0., 0.002))
    s2i = np.where(noice | (del_hi < 0), 0., r(0., 1e-4))
    # the young ice (after the column: M_h_young = hi_young * conc_young)
    cy, hiy, hsy = r(0.05, 0.2), r(0.06, 0.2), r(0.005, 0.02)
    m = is_("sc_not_filled")
    cy[m], hiy[m] = r(0.08, 0.12)[m], r(0.015, 0.03)[m]
    m = is_("sharp")
    hiy[m] = r(0.3, 0.4)[m]
    m = is_("no_room")
    cy[m] = r(0.03, 0.06)[m]
    m = is_("denom_clamp")
    cy[m] = r(0.01, 0.04)[m]
    cy[noice] = 0.
    del_hi_y = np.where(cy > 0, r(0.0005, 0.002), 0.)
    del_hi_y[melt] = -r(0.0005, 0.002)[melt]
    young_rows = {"Qio_young": None, "hi_young": hiy * (cy > 0), "hs_young": hsy * (cy > 0), "hi_young_old": (hiy - del_hi_y) * (cy > 0), "del_hi_young": del_hi_y,
                  "del_hs_young_mlt": np.where(cy > 0, -r(0., 0.001), 0.), "mlt_hi_top_young": np.where(del_hi_y < 0, 0.4 * del_hi_y, 0.),
                  "mlt_hi_bot_young": np.where(del_hi_y < 0, 0.6 * del_hi_y, 0.), "del_hi_s2i_young": np.where((cy > 0) & (del_hi_y > 0), r(0., 5e-5), 0.)}
    Qio = (inp["sst"] - tfrw) * float(rhow) * float(cpw) * 9. / DT
    young_rows["Qio_young"] = Qio.copy()
    precip = r(0., 3e-5)
    precip[is_("pond_frozen")] = 0.                    # (no water but the little the pond holds: the lid that forms takes all of it)
    snowfall = precip * np.where(rng.random(Ne) < 0.3, 0., r(0.2, 1.))
    col = {"snowfall": snowfall, "Qdw": r(-2., 2.), "Fdw": r(-1e-6, 1e-6), "tfrw": tfrw, "Qio": Qio, "hi": hi, "hs": hs, "hi_old": hi_old, "del_hi": del_hi,
           "del_hs_mlt": del_hs_mlt, "mlt_hi_top": mlt_top, "mlt_hi_bot": mlt_bot, "del_hi_s2i": s2i}
    col.update(young_rows)
    for k in _abi.COL_ROWS:
        inp["K:" + k] = col[k]
    Qia = np.where(rng.random(Ne) < 0.5, 1., -1.) * r(20., 80.)
    Qia[is_("pond_lid_forms", "pond_frozen")] = r(20., 80.)[is_("pond_lid_forms", "pond_frozen")]
    flux = {"Qow": Qow, "Qlw_ow": r(30., 60.), "Qsw_ow": -r(0., 200.), "Qlh_ow": r(0., 30.), "Qsh_ow": r(-10., 30.), "evap": r(0., 2e-5), "tau_ow": r(0., 0.1),
            "Qia": Qia, "Qlwi": r(20., 60.), "Qswi": -r(0., 100.), "Qlhi": r(0., 10.), "Qshi": r(-10., 20.), "I": r(0., 5.), "subl": r(0., 1e-6), "dQiadT": r(10., 20.),
            "albedo": r(0.5, 0.85)}
    for k in _abi.FLUX_ICE_ROWS:
        flux[k + "_young"] = {"Qia": r(20., 80.), "Qlw": r(20., 60.), "Qsw": -r(0., 100.), "Qlh": r(0., 10.), "Qsh": r(-10., 20.), "I": r(0., 5.), "subl": r(0., 1e-6),
                              "dQiadT": r(10., 20.), "albedo": r(0.3, 0.6)}[k]
    for k in _abi.FLUX_ROWS:
        inp["F:" + k] = flux[k]
    inp["precip"] = precip
    inp["mld"] = r(8., 40.)
    conc_upd = np.where(rng.random(Ne) < 0.3, 0., r(0.001, 0.05))
    m = is_("assim_neg")
    conc_upd[m] = -r(0.05, 0.2)[m]
    conc_upd[noice] = np.where(rng.random(Ne) < 0.5, 0., -r(0.05, 0.2))[noice]    # (ice assimilated away altogether: pow(0, n))
    inp["conc_upd"] = conc_upd
    # the state
    inp.update(conc=conc, thick=conc * hi_old, snow_thick=conc * hs, ridge_ratio=np.where(noice, 0., r(0.1, 0.5)), conc_young=cy, h_young=cy * hiy, hs_young=cy * hsy)
    cmyi = r(0.2, 0.9) * conc
    cmyi[is_("melt_nomyi")] = 0.
    inp.update(conc_myi=cmyi, thick_myi=cmyi * hi_old * r(0.9, 1.), time_relaxation_damage=r(1e6, 3e6))
    pf, lid, pv = np.zeros(Ne), np.zeros(Ne), np.zeros(Ne)
    m = is_("pond_lid")
    lid[m], pv[m], pf[m] = r(0.01, 0.02)[m], r(0.05, 0.1)[m], r(0.2, 0.3)[m]
    m = is_("pond_lid_forms")
    pv[m], pf[m] = r(0.05, 0.1)[m], r(0.2, 0.3)[m]
    m = is_("pond_thick_lid")
    lid[m], pv[m], pf[m] = r(0.1, 0.12)[m], r(0.05, 0.06)[m], r(0.2, 0.3)[m]
    m = is_("pond_frozen")
    pv[m], pf[m] = r(1e-5, 3e-5)[m], r(0.001, 0.002)[m]
    inp.update(pond_fraction=pf, lid_volume=lid, pond_volume=pv)
    inp.update(tice0=r(-20., -5.), tice1=r(-10., -3.), tice2=r(-5., -2.5))
    fd = rng.integers(0, 2, Ne).astype(float)
    onset = rng.integers(0, 2, Ne).astype(float)
    m = is_("fd_at_onset0")
    fd[m], onset[m] = 3., 0.
    m = is_("fd_at_onset1")
    fd[m], onset[m] = np.where(rng.random(Ne) < 0.5, 3., 5.)[m], 1.
    m = is_("fd_below")
    fd[m], onset[m] = 2., 0.
    inp.update(del_vi_tend=np.where(rng.random(Ne) < 0.5, 1., -1.) * r(0.01, 0.05), freeze_days=fd, freeze_onset=onset, conc_summer=r(0.2, 0.5) * (~noice),
               thick_summer=r(0.3, 0.9) * (~noice), fyi_fraction=r(0., 0.5) * conc, age_det=r(1e6, 5e7) * (~noice), age=r(1e6, 5e7) * (~noice))
    return {k: np.ascontiguousarray(v, np.float64) for k, v in inp.items()}, s, calm


def blank_inputs(Ne, Nn, **rows):
    """every row zero but those given (scalars are broadcast): the hand-computed columns of tests/test_slab_ref.py"""
    inp = {k: np.zeros(Ne) for k in FLUX + COL + IN_PLACE + ("precip", "mld", "conc_upd")}
    inp["wind"] = np.zeros(2 * Nn)
    for k, v in rows.items():
        assert k in inp, k
        inp[k] = np.full(inp[k].shape, v, np.float64) if np.ndim(v) == 0 else np.ascontiguousarray(v, np.float64)
    return inp


def moved_one_ulp(inp, direction):
    """every input moved to the neighbouring double away from (+1) or towards (-1) zero.  A value that is a value of its own stays: a zero (no ice, no snow, no
    pond), an exact one (a full cell: std::min(1., ...) makes it), the counters freeze_days and freeze_onset (whole numbers by construction: += 1., std::round);
    the calm nodes stay calm (their wind is zero)."""
    out = {}
    for k, v in inp.items():
        if k in ("freeze_days", "freeze_onset"):
            out[k] = v.copy()
            continue
        target = np.where(v > 0, np.inf, -np.inf) if direction > 0 else np.zeros(v.shape)
        out[k] = np.where((v == 0.) | (v == 1.), v, np.nextafter(v, target))
    return out


def edge_of_the_reference(inp, cfg, words):
    """The one decision of the scope that sits on an edge by the reference's own arithmetic: in a cell without young ice newice_type 4 sets M_conc_young =
    newice / h_young_min and then asks M_h_young (= newice) < h_young_min * M_conc_young (FE.cpp:5508, 5515) -- the rounding of x * (y / x) decides, and both
    sides give the same bits (M_conc_young = M_h_young / h_young_min either way; the other side's hi = h_young_min is far below h_young_max_sharp).  Returns the
    words with that bit cleared on those elements, which is what the robustness checks compare."""
    w = words.copy()
    if int(cfg["newice_type"]) == 4:
        w[(inp["conc_young"] == 0.) & (inp["h_young"] == 0.)] &= np.uint32(~BIT["n4_not_filled"] & 0xFFFFFFFF)
    return w


def copy(inp):
    return {k: v.copy() for k, v in inp.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def clock(**flags):
    c = dict(NO_CLOCK)
    for k, v in flags.items():
        if k not in c:
            raise KeyError(k)
        c[k] = int(v)
    return c


# ---- what tests/test_gpu_slab.py and scripts share: a handle fed with the designed inputs, the device_rows doors, one fluxes -> column -> slab round
def hip():
    """the HIP runtime the library itself has loaded: hipMemcpy is the way through the device_rows doors (None: not found)"""
    from nextsim_amd import dynamics
    dynamics.load_library()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = ctypes.CDLL(line.split()[-1])
            lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            lib.hipMemcpy.restype = ctypes.c_int
            return lib
    return None


def sane_inputs(inp, f):
    """make_inputs' rows bent to a case's own ice state f (tests that go on to a dynamics step): the state rows are the case's, the column's hi_old, hi, hs follow
    from them, the growth stays small and nothing melts away"""
    out = copy(inp)
    for k in ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "ridge_ratio", "conc_myi", "thick_myi", "time_relaxation_damage"):
        out[k] = np.ascontiguousarray(f[k], np.float64).copy()
    conc, ice = out["conc"], out["conc"] > 0
    safe = np.where(ice, conc, 1.)
    hi_old = np.where(ice, out["thick"] / safe, 0.)
    del_hi = np.where(hi_old > 0.2, np.clip(inp["K:del_hi"], -0.01, 0.01), np.where(ice, 0.001, 0.))
    out["K:hi_old"], out["K:del_hi"], out["K:hi"], out["K:hs"] = hi_old, del_hi, hi_old + del_hi, np.where(ice, out["snow_thick"] / safe, 0.)
    for k in ("K:mlt_hi_top", "K:mlt_hi_bot"):
        out[k] = np.where(del_hi < 0, 0.5 * del_hi, 0.)
    out["K:del_hi_young"] = np.where(out["conc_young"] > 0, np.abs(inp["K:del_hi_young"]), 0.)
    for k in ("K:mlt_hi_top_young", "K:mlt_hi_bot_young"):
        out[k] = np.zeros_like(conc)
    return {k: np.ascontiguousarray(v, np.float64) for k, v in out.items()}


def gpu_handle(p, lm, f, inp, finp, ccfg, cfg=None, put=SLAB_STATE + ("conc_upd",)):
    """A handle on the local mesh lm whose ice state and wind are the slab inputs `inp` (the rest of the state and the forcing stay the case's f), the fluxes
    configured and fed (the atmosphere of fluxes_ref.make_inputs `finp`), the column configured (ccfg) and fed, the slab configured (cfg: a dict of
    default_config(), None = not configured) and the rows named in `put` given.  Returns the handle and the state dict it was given."""
    from nextsim_amd import dynamics
    f = dict(f, **{k: inp[k].copy() for k in STATE[:-1]}, wind=inp["wind"].copy(), time_relaxation_damage=inp["time_relaxation_damage"].copy())
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1))   # (the drags stay: a later step must not see that fluxes() ran)
    feed_flux_state(fe, inp, finp)
    fe.column_configure(**ccfg)
    fe.column_set_forcing(precip=inp["precip"], snow=np.ones_like(inp["precip"]), ocean_temp=inp["sst"], ocean_salt=inp["sss"], mld=inp["mld"])
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    if cfg is not None:
        fe.slab_configure(**cfg)
        fe.slab_put(**{k: inp[k] for k in put})
    return fe, f


def feed_flux_state(fe, inp, finp):
    fe.flux_set_atmosphere(tair=finp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"])
    fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], sst=inp["sst"], sss=inp["sss"], pond_fraction=inp["pond_fraction"],
                       lid_volume=inp["lid_volume"]))


def _write_rows(fe, lib, dev, rows):
    for k, a in rows.items():
        a = np.ascontiguousarray(a, np.float64)
        assert dev[k] and a.size == fe.lm.num_elements
        assert lib.hipMemcpy(dev[k], a.ctypes.data, a.nbytes, 1) == 0


def device_state(fe):
    """every row the slab writes in place, from the device"""
    st = fe.get_state()
    out = {k: st[k] for k in STATE[:-1]}
    out.update(fe.slab_get(SLAB_STATE + ("time_relaxation_damage",)))
    out.update(fe.flux_get(FLUX_STATE + ("tice0",)))
    out.update(fe.column_get())
    return out


def gpu_round(fe, f, ref, dt, clock):
    """fluxes() -> column(dt) -> slab(dt, clock) on the device, with the designed flux rows AND column rows of `ref` written through the two device_rows doors
    before the slab runs, and the rows the column itself moved (tice0, tice1, tice2, h_young, hs_young) put back to ref's: the slab then runs on ref's bits, and
    neither earlier slice's tolerance enters.  Returns (the 29 rows, the rows written in place, the branch words, the flux rows before and after the slab)."""
    lib = hip()
    assert lib is not None, "the HIP runtime of the library was not found: no way through the device_rows doors"
    fe.fluxes()
    _, fdev = fe.fluxes_get((), want_device=True)
    fe.synchronize()
    _write_rows(fe, lib, fdev, {k[2:]: ref[k] for k in FLUX if k != "F:tau_ow"})
    fe.column(dt)
    _, kdev = fe.column_rows((), want_device=True)
    fe.synchronize()
    _write_rows(fe, lib, kdev, {k[2:]: ref[k] for k in COL})
    fe.put_state(dict(f, **{k: ref[k] for k in STATE}))
    fe.flux_put(tice0=ref["tice0"])
    fe.column_put(tice1=ref["tice1"], tice2=ref["tice2"])
    before = fe.fluxes_get()
    fe.slab(dt, clock)
    rows = fe.slab_rows()
    words = fe.debug_array("slab_branches").astype(np.uint32)
    after = fe.fluxes_get()
    return rows, device_state(fe), words, before, after
